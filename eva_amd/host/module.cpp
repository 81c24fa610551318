// module.cpp — pybind11 module eva_amd._eva: the same Python-visible surface as the reference's
// eva._eva (/root/reference/python/eva/wrapper.cpp:26-246) over the arena IR, the CKKS compiler
// and the MI355X executor.  Submodules: _ckks (compiler), _seal (backend; the name is kept so
// `from eva.seal import generate_keys` keeps working — the backend behind it is libeva_hip.so).
#include <pybind11/numpy.h>
#include <chrono>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "executor.h"
#include "serialization.h"

namespace py = pybind11;
using namespace evahost;

namespace {

struct PyTerm {
  Program *prog;
  TermId id;
  py::object owner; // keeps the owning Program alive while a handle exists
};

std::vector<TermId> ids_of(const std::vector<PyTerm> &v) {
  std::vector<TermId> out;
  for (auto &t : v) out.push_back(t.id);
  return out;
}

template <class Vec> py::array_t<uint64_t> to_numpy(const Vec &v, std::vector<py::ssize_t> shape) {
  py::array_t<uint64_t> a(shape);
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(u64));
  return a;
}

static int g_num_threads = 1;

// the arrays of encrypt_array as the library takes them: C-contiguous [B][n] of float64, float32 or uint8 — what
// eva_amd.seal.normalise_arrays hands over (it converts everything else), so anything else here is an error
std::map<std::string, ArrayView> array_views(const std::map<std::string, py::array> &arrays) {
  std::map<std::string, ArrayView> out;
  for (auto &kv : arrays) {
    const py::array &a = kv.second;
    const char kind = a.dtype().kind();
    ArrayView v;
    if (kind == 'f' && a.itemsize() == 8) v.dtype = EVAH_F64;
    else if (kind == 'f' && a.itemsize() == 4) v.dtype = EVAH_F32;
    else if (kind == 'u' && a.itemsize() == 1) v.dtype = EVAH_U8;
    else throw std::invalid_argument("input " + kv.first + ": the array must be float64, float32 or uint8");
    if (a.ndim() != 2 || !(a.flags() & py::array::c_style)) throw std::invalid_argument("input " + kv.first + ": the array must be C-contiguous [B, n]");
    v.data = a.data();
    v.B = (size_t)a.shape(0);
    v.n = (size_t)a.shape(1);
    out.emplace(kv.first, v);
  }
  return out;
}

// the device arrays of encrypt_array as eva_amd.seal.normalise_device_arrays hands them over:
// {name: (device pointer, EVAH_* code, B, n, row pitch in bytes, producer stream or 0)}, added to the host views
using DevArrayArgs = std::map<std::string, std::tuple<uintptr_t, int, size_t, size_t, size_t, uintptr_t>>;
std::map<std::string, ArrayView> with_device_arrays(std::map<std::string, ArrayView> views, const DevArrayArgs &dev) {
  for (auto &kv : dev) {
    if (views.count(kv.first)) throw std::invalid_argument("encrypt_array: input " + kv.first + " is given twice");
    ArrayView v;
    v.data = reinterpret_cast<const void *>(std::get<0>(kv.second));
    v.dtype = std::get<1>(kv.second);
    if (v.dtype != EVAH_F64 && v.dtype != EVAH_F32 && v.dtype != EVAH_U8) throw std::invalid_argument("input " + kv.first + ": the array must be float64, float32 or uint8");
    v.B = std::get<2>(kv.second);
    v.n = std::get<3>(kv.second);
    v.pitch = std::get<4>(kv.second);
    v.on_device = true;
    v.producer = reinterpret_cast<void *>(std::get<5>(kv.second));
    views.emplace(kv.first, v);
  }
  return views;
}
// decrypt_array's rule for uint8 on values the host holds: np.clip(np.rint(np.nan_to_num(a, nan=0)), 0, 255).astype(uint8)
py::array as_uint8(const py::array &a) {
  py::module_ np = py::module_::import("numpy");
  return py::array(np.attr("clip")(np.attr("rint")(np.attr("nan_to_num")(a, py::arg("nan") = 0.0)), 0, 255).attr("astype")(np.attr("uint8")));
}

} // namespace

PYBIND11_MODULE(_eva, m) {
  m.doc() = "MI355X-native EVA: Python wrapper";

  py::enum_<Op>(m, "Op")
      .value("Undef", Op::Undef).value("Input", Op::Input).value("Output", Op::Output).value("Constant", Op::Constant)
      .value("Negate", Op::Negate).value("Add", Op::Add).value("Sub", Op::Sub).value("Mul", Op::Mul)
      .value("RotateLeftConst", Op::RotateLeftConst).value("RotateRightConst", Op::RotateRightConst)
      .value("Relinearize", Op::Relinearize).value("ModSwitch", Op::ModSwitch).value("Rescale", Op::Rescale)
      .value("Encode", Op::Encode);
  py::enum_<Type>(m, "Type")
      .value("Undef", Type::Undef).value("Cipher", Type::Cipher).value("Raw", Type::Raw).value("Plain", Type::Plain);

  py::class_<PyTerm>(m, "Term", "Native Term handle")
      .def_property_readonly("op", [](const PyTerm &t) { return t.prog->at(t.id).op; }, "The operation performed by this term")
      .def_property_readonly("index", [](const PyTerm &t) { return t.id; });

  py::class_<Program>(m, "Program", "Native Program class")
      .def(py::init<std::string, uint64_t>(), py::arg("name"), py::arg("vec_size"))
      .def_property("name", &Program::name, &Program::set_name, "The name of this program")
      .def_property_readonly("vec_size", &Program::vec_size, "The number of elements for all vectors in this program")
      .def_property_readonly("inputs", [](py::object self) {
        Program &p = self.cast<Program &>();
        std::unordered_map<std::string, PyTerm> out;
        for (auto &kv : p.inputs()) out.emplace(kv.first, PyTerm{&p, kv.second, self});
        return out;
      }, "A dictionary from input names to terms")
      .def_property_readonly("outputs", [](py::object self) {
        Program &p = self.cast<Program &>();
        std::unordered_map<std::string, PyTerm> out;
        for (auto &kv : p.outputs()) out.emplace(kv.first, PyTerm{&p, kv.second, self});
        return out;
      }, "A dictionary from output names to terms")
      .def("set_output_ranges", [](Program &p, uint32_t range) {
        for (auto &kv : p.outputs()) { p.at(kv.second).has_range = true; p.at(kv.second).range = range; }
      }, py::arg("range"), "Sets the range (in bits) all outputs must accommodate")
      .def("set_input_scales", [](Program &p, uint32_t scale) {
        for (TermId s : p.sources()) { p.at(s).has_encode_scale = true; p.at(s).encode_scale = scale; }
      }, py::arg("scale"), "Sets the scale (in bits) all inputs and constants are encoded at")
      .def("to_DOT", &Program::to_dot)
      .def("_make_term", [](py::object self, Op op, const std::vector<PyTerm> &operands) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_term(op, ids_of(operands)), self}; })
      .def("_make_left_rotation", [](py::object self, const PyTerm &t, int32_t s) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_left_rotation(t.id, s), self}; })
      .def("_make_right_rotation", [](py::object self, const PyTerm &t, int32_t s) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_right_rotation(t.id, s), self}; })
      .def("_make_dense_constant", [](py::object self, std::vector<double> v) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_dense_constant(std::move(v)), self}; })
      .def("_make_uniform_constant", [](py::object self, double v) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_uniform_constant(v), self}; })
      .def("_make_input", [](py::object self, const std::string &name, Type t) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_input(name, t), self}; })
      .def("_make_output", [](py::object self, const std::string &name, const PyTerm &t) { Program &p = self.cast<Program &>(); return PyTerm{&p, p.make_output(name, t.id), self}; })
      // introspection used by the parity tests: the live DAG in topological order
      .def("_dump", [](Program &p) {
        py::list out;
        for (TermId t : p.topo_order()) {
          const Term &x = p.at(t);
          py::dict d;
          d["id"] = t;
          d["op"] = x.op;
          d["operands"] = x.operands;
          if (x.has_rotation) d["rotation"] = x.rotation;
          if (x.has_rescale_divisor) d["rescale_divisor"] = x.rescale_divisor;
          if (x.has_type) d["type"] = x.type_attr;
          if (x.has_range) d["range"] = x.range;
          if (x.has_encode_scale) d["encode_scale"] = x.encode_scale;
          if (x.has_encode_level) d["encode_level"] = x.encode_level;
          if (x.constant) d["constant"] = x.constant->values;
          out.append(d);
        }
        return out;
      });

  m.def("evaluate", &evaluate, py::arg("program"), py::arg("inputs"), "Evaluate the program without homomorphic encryption (reference semantics)");
  // serialization (wrapper.cpp:110-116)
  // Program / CKKSParameters / CKKSSignature: the reference's protobuf wire format by default (files
  // interchange with microsoft/EVA); format="native" = this repo's container
  auto want_wire = [](const std::string &format) {
    if (format == "eva") return true;
    if (format == "native") return false;
    throw std::invalid_argument("format must be 'eva' or 'native'");
  };
  m.def("save", [want_wire](const Program &o, const std::string &path, const std::string &format) {
    if (want_wire(format)) save_wire_to_file("Program", wire::encode(o), path);
    else save_to_file(Kind::Program, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "eva");
  m.def("save", [want_wire](const CKKSParameters &o, const std::string &path, const std::string &format) {
    if (want_wire(format)) save_wire_to_file("CKKSParameters", wire::encode(o), path);
    else save_to_file(Kind::Parameters, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "eva");
  m.def("save", [want_wire](const CKKSSignature &o, const std::string &path, const std::string &format) {
    if (want_wire(format)) save_wire_to_file("CKKSSignature", wire::encode(o), path);
    else save_to_file(Kind::Signature, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "eva");
  // valuations and key contexts: this repo's container by default; format="seal" (or "seal+zlib" / "seal+zstd") = the
  // reference's protobuf messages around SEAL's binary object format (seal.proto, seal_format.h)
  auto seal_compr = [](const std::string &format, bool &seal) {
    seal = true;
    if (format == "seal") return sealfmt::None;
    if (format == "seal+zlib") return sealfmt::Zlib;
    if (format == "seal+zstd") return sealfmt::Zstd;
    seal = false;
    if (format == "native") return sealfmt::None;
    throw std::invalid_argument("format must be 'native', 'seal', 'seal+zlib' or 'seal+zstd'");
  };
  m.def("save", [seal_compr](const HipValuation &o, const std::string &path, const std::string &format) {
    bool seal = false;
    const sealfmt::Compr c = seal_compr(format, seal);
    if (seal) save_wire_to_file("SEALValuation", sealfmt::encode_valuation(o, c), path);
    else save_to_file(Kind::Valuation, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "native");
  m.def("save", [seal_compr](const HipPublic &o, const std::string &path, const std::string &format) {
    bool seal = false;
    const sealfmt::Compr c = seal_compr(format, seal);
    // the SEAL format keeps refusing every collective context: without the key of DESIGN.md 1.15 it lacks what SEAL's
    // RelinKeys needs, and with it the file could not say `collective` or name the dropped Galois elements
    if (seal && o.collective && !o.has_relin_key())
      throw std::invalid_argument("a collective context has no relinearization key, which the SEAL format requires: save it with format='native'");
    if (seal && o.collective)
      throw std::invalid_argument("the SEAL format cannot mark a context as collective or name its dropped Galois elements: save it with format='native'");
    if (seal) save_wire_to_file("SEALPublic", sealfmt::encode_public(o, c), path);
    else save_to_file(Kind::Public, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "native");
  m.def("save", [seal_compr](const HipSecret &o, const std::string &path, const std::string &format) {
    bool seal = false;
    const sealfmt::Compr c = seal_compr(format, seal);
    if (seal) save_wire_to_file("SEALSecret", sealfmt::encode_secret(o, c), path);
    else save_to_file(Kind::Secret, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "native");
  // a re-key key has this repo's container only: SEAL has no such object
  m.def("save", [seal_compr](const RekeyKey &o, const std::string &path, const std::string &format) {
    bool seal = false;
    (void)seal_compr(format, seal);
    if (seal) throw std::invalid_argument("a RekeyKey has no SEAL format: save it with format='native'");
    save_to_file(Kind::RekeyKey, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "native");
  // decryption shares have this repo's container only (kind 8): SEAL has no such object
  m.def("save", [seal_compr](const DecryptionShares &o, const std::string &path, const std::string &format) {
    bool seal = false;
    (void)seal_compr(format, seal);
    if (seal) throw std::invalid_argument("DecryptionShares have no SEAL format: save them with format='native'");
    save_to_file(Kind::Shares, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "native");
  // a share of the collective relinearization-key generation has this repo's container only (kind 9)
  m.def("save", [seal_compr](const RelinShare &o, const std::string &path, const std::string &format) {
    bool seal = false;
    (void)seal_compr(format, seal);
    if (seal) throw std::invalid_argument("a RelinShare has no SEAL format: save it with format='native'");
    save_to_file(Kind::RelinShare, o, path);
  }, py::arg("obj"), py::arg("path"), py::arg("format") = "native");
  // test hooks of the SEAL object format
  m.def("_blake2b_256", [](py::bytes data) {
    const std::string s = data;
    uint8_t out[32];
    sealfmt::blake2b(out, 32, (const uint8_t *)s.data(), s.size());
    return py::bytes((const char *)out, 32);
  });
  m.def("_seal_zstd_available", []() { return sealfmt::ZstdLib::get().ok(); });
  // one SEAL object (the bytes of a SEALObject.data) from raw words: what tests/golden/export_seal_vectors.py hands to
  // tools/seal_parity.cpp, which loads them with SEAL itself and compares SEAL's own save() with them
  m.def("_seal_blob", [](const std::string &kind, uint32_t N, const std::vector<uint64_t> &primes,
                         py::array_t<uint64_t, py::array::c_style | py::array::forcecast> data, double scale) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    const u64 *d = (const u64 *)data.data();
    auto shape_is = [&](std::initializer_list<py::ssize_t> want) {
      if ((size_t)data.ndim() != want.size()) throw std::invalid_argument("wrong number of dimensions for a SEAL " + kind);
      size_t i = 0;
      for (py::ssize_t w : want) {
        if (w >= 0 && data.shape(i) != w) throw std::invalid_argument("wrong shape for a SEAL " + kind);
        i++;
      }
    };
    std::string out;
    if (kind == "parms") out = sealfmt::parms_obj(h, sealfmt::None);
    else if (kind == "ciphertext") { shape_is({-1, -1, (py::ssize_t)N}); out = sealfmt::ciphertext_obj(h, (uint32_t)data.shape(0), (uint32_t)data.shape(1), scale, d, sealfmt::None); }
    else if (kind == "plaintext") { shape_is({-1, (py::ssize_t)N}); out = sealfmt::plaintext_obj(h, (uint32_t)data.shape(0), scale, d, sealfmt::None); }
    else if (kind == "public_key") { shape_is({2, (py::ssize_t)h.k, (py::ssize_t)N}); out = sealfmt::public_key_obj(h, d, sealfmt::None); }
    else if (kind == "secret_key") { shape_is({(py::ssize_t)h.k, (py::ssize_t)N}); out = sealfmt::secret_key_obj(h, d, sealfmt::None); }
    else if (kind == "relin_keys") {
      shape_is({-1, 2, (py::ssize_t)h.k, (py::ssize_t)N});
      SwitchKey k;
      k.n_digits = (uint32_t)data.shape(0);
      k.data.assign(d, d + data.size());
      out = sealfmt::kswitch_obj(h, 1, {{0, &k}}, sealfmt::None);
    } else throw std::invalid_argument("unknown SEAL object kind " + kind);
    return py::bytes(out);
  }, py::arg("kind"), py::arg("N"), py::arg("primes"), py::arg("data"), py::arg("scale") = 1.0);
  m.def("_seal_galois_blob", [](uint32_t N, const std::vector<uint64_t> &primes, const std::map<uint32_t, py::array_t<uint64_t, py::array::c_style | py::array::forcecast>> &keys) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    std::map<uint64_t, SwitchKey> own;
    for (auto &kv : keys) {
      if (kv.second.ndim() != 4 || kv.second.shape(1) != 2 || kv.second.shape(2) != (py::ssize_t)h.k || kv.second.shape(3) != (py::ssize_t)N || !(kv.first & 1) || kv.first >= 2 * N)
        throw std::invalid_argument("wrong shape / element for a SEAL Galois key");
      SwitchKey k;
      k.n_digits = (uint32_t)kv.second.shape(0);
      k.data.assign((const u64 *)kv.second.data(), (const u64 *)kv.second.data() + kv.second.size());
      own.emplace((uint64_t)(kv.first - 1) / 2, std::move(k));
    }
    std::map<uint64_t, const SwitchKey *> slots;
    for (auto &kv : own) slots.emplace(kv.first, &kv.second);
    return py::bytes(sealfmt::kswitch_obj(h, N, slots, sealfmt::None));
  }, py::arg("N"), py::arg("primes"), py::arg("keys"));
  m.def("load", [](const std::string &path) -> py::object {
    KnownType k = load_from_file(path);
    if (auto *p = std::get_if<std::unique_ptr<Program>>(&k)) return py::cast(std::move(*p));
    if (auto *p = std::get_if<CKKSParameters>(&k)) return py::cast(*p);
    if (auto *p = std::get_if<CKKSSignature>(&k)) return py::cast(*p);
    if (auto *p = std::get_if<HipValuation>(&k)) return py::cast(std::move(*p));
    if (auto *p = std::get_if<std::shared_ptr<HipPublic>>(&k)) return py::cast(*p);
    if (auto *p = std::get_if<std::shared_ptr<RekeyKey>>(&k)) return py::cast(*p);
    if (auto *p = std::get_if<std::shared_ptr<DecryptionShares>>(&k)) return py::cast(*p);
    if (auto *p = std::get_if<std::shared_ptr<RelinShare>>(&k)) return py::cast(*p);
    return py::cast(std::get<std::shared_ptr<HipSecret>>(k));
  }, py::arg("path"), "Load a previously saved object (same class as was saved)");

  m.def("set_num_threads", [](int n) { if (n < 1) throw std::invalid_argument("num_threads must be positive"); g_num_threads = n; }, py::arg("num_threads"),
        "Node-level parallelism of execute(): contexts made by generate_keys() afterwards spread independent DAG nodes over min(n, 8) "
        "issue queues (HIP streams) — the GPU counterpart of the reference's Galois worker threads; 1 (the default) = one in-order queue");
  struct GaloisGuard {};
  py::class_<GaloisGuard>(m, "_GaloisGuard").def(py::init());

  // ---- CKKS compiler
  py::module mckks = m.def_submodule("_ckks", "CKKS compiler");
  py::class_<CKKSCompiler>(mckks, "CKKSCompiler")
      .def(py::init(), "Create a compiler with the default config")
      .def(py::init([](const std::unordered_map<std::string, std::string> &cfg) { return CKKSCompiler(CKKSConfig(cfg)); }), py::arg("config"))
      .def("compile", [](CKKSCompiler &c, Program &p) {
        auto r = c.compile(p);
        return py::make_tuple(py::cast(std::move(std::get<0>(r))), std::get<1>(r), std::get<2>(r));
      }, py::arg("program"));
  py::class_<CKKSParameters>(mckks, "CKKSParameters", "Abstract encryption parameters for CKKS")
      .def(py::init([](std::vector<uint32_t> bits, std::set<int> rot, uint32_t n) { CKKSParameters p; p.prime_bits = bits; p.rotations = rot; p.poly_modulus_degree = n; return p; }),
           py::arg("prime_bits"), py::arg("rotations"), py::arg("poly_modulus_degree"))
      .def_readwrite("prime_bits", &CKKSParameters::prime_bits)
      .def_readwrite("rotations", &CKKSParameters::rotations)
      .def_readwrite("poly_modulus_degree", &CKKSParameters::poly_modulus_degree);
  // (both can be made by hand: a refresh may target any level and scale of the chain, not only what a compiled program
  // on this machine asks for)
  py::class_<CKKSEncodingInfo>(mckks, "CKKSEncodingInfo")
      .def(py::init([](Type t, int scale, int level) { return CKKSEncodingInfo{t, scale, level}; }), py::arg("input_type"), py::arg("scale"),
           py::arg("level"))
      .def_readonly("input_type", &CKKSEncodingInfo::input_type)
      .def_readonly("scale", &CKKSEncodingInfo::scale)
      .def_readonly("level", &CKKSEncodingInfo::level);
  py::class_<CKKSSignature>(mckks, "CKKSSignature")
      .def(py::init([](int vec_size, std::unordered_map<std::string, CKKSEncodingInfo> inputs) {
             CKKSSignature s;
             s.vec_size = vec_size;
             s.inputs = std::move(inputs);
             return s;
           }), py::arg("vec_size"), py::arg("inputs"))
      .def_readonly("vec_size", &CKKSSignature::vec_size)
      .def_readonly("inputs", &CKKSSignature::inputs);

  // ---- backend
  py::module mseal = m.def_submodule("_seal", "MI355X CKKS execution backend (drop-in for eva._eva._seal)");
  // devices / shard: several GPUs behind one execute() (eva_amd/host/multi_device.h); the defaults come from
  // EVA_NUM_GPUS / EVA_DEVICES / EVA_SHARD.  set_num_threads(n) — the reference's size of the parallel
  // traversal (wrapper.cpp:128-137) — is the number of issue queues independent DAG nodes are spread over.
  // compress_keys: the evaluation keys as c0 + a 32-byte seed per digit, expanded on the GPU at upload
  // device_keygen: the same compressed keys, generated on the GPU from the secret key and the host's draws
  // device_sampling: every polynomial of the key set from a 32-byte key of its own, drawn on the GPU with device_keygen
  mseal.def("generate_keys", [](const CKKSParameters &p, uint64_t seed, py::object devices, py::object shard, bool compress_keys, bool device_keygen,
                                bool device_sampling, py::object common_seed) {
    // devices / shard reach generate_keys before any key is made: device key generation runs on member 0's device
    std::vector<int> dv;
    std::string sh;
    if (!devices.is_none()) dv = devices.cast<std::vector<int>>();
    if (!shard.is_none()) sh = shard.cast<std::string>();
    std::array<uint8_t, 32> cs{};
    if (!common_seed.is_none()) {
      const std::string k = common_seed.cast<py::bytes>();
      if (k.size() != 32) throw std::invalid_argument("common_seed is 32 bytes");
      std::memcpy(cs.data(), k.data(), 32);
    }
    auto kp = generate_keys(p, seed, compress_keys, device_keygen, devices.is_none() ? nullptr : &dv, shard.is_none() ? nullptr : &sh, device_sampling,
                            common_seed.is_none() ? nullptr : &cs);
    if (g_num_threads > 1) kp.first->num_queues = std::min(g_num_threads, 8);
    return kp;
  }, py::arg("abstract_params"), py::arg("seed") = 0, py::arg("devices") = py::none(), py::arg("shard") = py::none(),
     py::arg("compress_keys") = false, py::arg("device_keygen") = false, py::arg("device_sampling") = false, py::arg("common_seed") = py::none());
  mseal.def("combine_public_contexts", [](const std::vector<std::shared_ptr<HipPublic>> &ctxs, py::object r1, py::object r2) {
    if (r1.is_none() != r2.is_none()) throw std::invalid_argument("combine_public_contexts: relin_round1 and relin_round2 go together: give both or neither");
    if (r1.is_none()) return combine_public_contexts(ctxs);
    const auto agg = r1.cast<std::shared_ptr<RelinShare>>();
    std::vector<std::shared_ptr<const RelinShare>> g;
    for (auto &s : r2.cast<std::vector<std::shared_ptr<RelinShare>>>()) g.push_back(s);
    return combine_public_contexts(ctxs, agg, &g);
  }, py::arg("public_contexts"), py::arg("relin_round1") = py::none(), py::arg("relin_round2") = py::none(),
            "The collective public context of parties whose keys were made with one generate_keys(..., common_seed=) (DESIGN.md 1.14): "
            "public key and the Galois keys present in all contexts under the sum of the parties' secrets. relin_round1 (the "
            "combine_relin_shares aggregate) and relin_round2 (one SEALSecret.relin_round2 share per context) go together and give it the "
            "collective relinearization key (DESIGN.md 1.15); without them it has none and executes everything but relinearize. "
            "It encrypts, is a make_rekey_key target, and saves / loads");
  mseal.def("combine_relin_shares", [](const std::vector<std::shared_ptr<RelinShare>> &shares) {
    std::vector<std::shared_ptr<const RelinShare>> s(shares.begin(), shares.end());
    return combine_relin_shares(s);
  }, py::arg("round1_shares"),
            "The sum of the parties' round-1 shares of the collective relinearization key (DESIGN.md 1.15), itself a round-1 RelinShare: "
            "what every party's relin_round2 and combine_public_contexts(relin_round1=) take. Public: anyone may form it");
  // test hooks: the seed derivation and the host twins of evah_keygen_relin_round1 / _round2 (ckks_host.h) on raw words
  mseal.def("_relin_round_seeds", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> seeds) {
    if (seeds.ndim() != 2 || seeds.shape(1) != 32) throw std::invalid_argument("seeds are [digits][32] bytes");
    const std::vector<uint8_t> out = relin_round_seeds(std::vector<uint8_t>(seeds.data(), seeds.data() + seeds.size()));
    py::array_t<uint8_t> a({seeds.shape(0), (py::ssize_t)32});
    std::memcpy(a.mutable_data(), out.data(), out.size());
    return a;
  }, py::arg("relin_seeds"));
  mseal.def("_relin_round1_host", [](uint32_t N, const std::vector<uint64_t> &primes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> s_ntt,
                                     py::array_t<uint8_t, py::array::c_style | py::array::forcecast> seeds,
                                     py::array_t<uint8_t, py::array::c_style | py::array::forcecast> r1keys) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    if (seeds.ndim() != 2 || seeds.shape(1) != 32 || r1keys.ndim() != 2 || r1keys.shape(1) != 32 || r1keys.shape(0) != seeds.shape(0))
      throw std::invalid_argument("seeds and randomness keys are [digits][32] bytes");
    SecretKey sk;
    sk.s_ntt.assign((const u64 *)s_ntt.data(), (const u64 *)s_ntt.data() + s_ntt.size());
    const uint32_t D = (uint32_t)seeds.shape(0);
    std::vector<std::array<uint8_t, 32>> rk(D);
    for (uint32_t J = 0; J < D; J++) std::memcpy(rk[J].data(), r1keys.data() + (size_t)32 * J, 32);
    return to_numpy(relin_round1_host(h, sk, D, seeds.data(), rk.data()), {(py::ssize_t)D, 2, (py::ssize_t)h.k, (py::ssize_t)N});
  }, py::arg("N"), py::arg("primes"), py::arg("s_ntt"), py::arg("seeds"), py::arg("r1keys"));
  mseal.def("_relin_round2_host", [](uint32_t N, const std::vector<uint64_t> &primes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> s_ntt,
                                     py::array_t<uint64_t, py::array::c_style | py::array::forcecast> agg1,
                                     py::array_t<uint8_t, py::array::c_style | py::array::forcecast> r1keys,
                                     py::array_t<uint8_t, py::array::c_style | py::array::forcecast> r2keys) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    if (r1keys.ndim() != 2 || r1keys.shape(1) != 32 || r2keys.ndim() != 2 || r2keys.shape(1) != 32 || r1keys.shape(0) != r2keys.shape(0))
      throw std::invalid_argument("randomness keys are [digits][32] bytes");
    const uint32_t D = (uint32_t)r1keys.shape(0);
    if (agg1.ndim() != 4 || agg1.shape(0) != (py::ssize_t)D || agg1.shape(1) != 2 || agg1.shape(2) != (py::ssize_t)h.k || agg1.shape(3) != (py::ssize_t)N)
      throw std::invalid_argument("the aggregate is [digits][2][k][N]");
    SecretKey sk;
    sk.s_ntt.assign((const u64 *)s_ntt.data(), (const u64 *)s_ntt.data() + s_ntt.size());
    std::vector<std::array<uint8_t, 32>> k1(D), k2(D);
    for (uint32_t J = 0; J < D; J++) {
      std::memcpy(k1[J].data(), r1keys.data() + (size_t)32 * J, 32);
      std::memcpy(k2[J].data(), r2keys.data() + (size_t)32 * J, 32);
    }
    return to_numpy(relin_round2_host(h, sk, D, (const u64 *)agg1.data(), k1.data(), k2.data()), {(py::ssize_t)D, (py::ssize_t)h.k, (py::ssize_t)N});
  }, py::arg("N"), py::arg("primes"), py::arg("s_ntt"), py::arg("agg1"), py::arg("r1keys"), py::arg("r2keys"));
  py::class_<RelinShare, std::shared_ptr<RelinShare>>(mseal, "RelinShare",
                                                      "One party's public share of the collective relinearization-key generation, or the sum of the "
                                                      "round-1 shares (DESIGN.md 1.15): made by SEALSecret.relin_round1 / relin_round2 and "
                                                      "combine_relin_shares, taken by combine_public_contexts; saves and loads")
      .def_readonly("round", &RelinShare::round)
      .def_readonly("N", &RelinShare::N)
      .def_readonly("poly_modulus_degree", &RelinShare::N)
      .def_readonly("primes", &RelinShare::primes)
      .def_readonly("n_digits", &RelinShare::n_digits)
      .def("words", [](const RelinShare &s) {
        if (s.round == 1) return to_numpy(s.data, {(py::ssize_t)s.n_digits, 2, (py::ssize_t)s.primes.size(), (py::ssize_t)s.N});
        return to_numpy(s.data, {(py::ssize_t)s.n_digits, (py::ssize_t)s.primes.size(), (py::ssize_t)s.N});
      }, "round 1: [digits][2][k][N]; round 2: [digits][k][N]; NTT form")
      // test hook: a share from raw words, unchecked (what a file would be checked for is checked where the share is used)
      .def_static("_from_words", [](uint32_t round, const std::vector<uint64_t> &primes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> words) {
        if (words.ndim() < 3) throw std::invalid_argument("share words are [digits][2][k][N] or [digits][k][N]");
        auto s = std::make_shared<RelinShare>();
        s->round = round;
        s->n_digits = (uint32_t)words.shape(0);
        s->N = (uint32_t)words.shape(words.ndim() - 1);
        s->primes.assign(primes.begin(), primes.end());
        s->data.assign((const u64 *)words.data(), (const u64 *)words.data() + words.size());
        return s;
      }, py::arg("round"), py::arg("primes"), py::arg("words"));
  py::class_<RelinEphemeral, std::shared_ptr<RelinEphemeral>>(mseal, "RelinEphemeral",
                                                              "What a party keeps between relin_round1 and relin_round2 (DESIGN.md 1.15): the keys its u is "
                                                              "regenerated from. Secret (whoever learns it learns the party's secret key), opaque, serves one "
                                                              "relin_round2 of the context that made it, cannot be saved or pickled, wiped when used and when destroyed")
      .def_readonly("used", &RelinEphemeral::used)
      .def("__reduce__", [](const RelinEphemeral &) -> py::object { throw py::type_error("a RelinEphemeral cannot be pickled: it holds a party's ephemeral secret"); })
      .def("__reduce_ex__", [](const RelinEphemeral &, int) -> py::object { throw py::type_error("a RelinEphemeral cannot be pickled: it holds a party's ephemeral secret"); });
  // test hook: small polynomial p of a 32-byte randomness key (csprng.h sampled_small) -> int8 [N]
  mseal.def("_sampled_small", [](py::bytes rk, uint32_t p, uint32_t N) {
    const std::string k = rk;
    if (k.size() != 32) throw std::invalid_argument("a randomness key is 32 bytes");
    py::array_t<int8_t> out({(py::ssize_t)N});
    sampled_small((const uint8_t *)k.data(), p, N, out.mutable_data());
    return out;
  }, py::arg("rkey"), py::arg("p"), py::arg("N"));
  // test hooks of threshold decryption: the flooding noise of a 32-byte key (csprng.h flood_wide) -> int64
  // [N], and the host twins of evah_decrypt_share_handles / evah_decrypt_combine_rows (ckks_host.h) on raw words
  mseal.def("_flood_wide", [](py::bytes fk, uint32_t sigma, uint32_t N) {
    const std::string k = fk;
    if (k.size() != 32) throw std::invalid_argument("a flooding key is 32 bytes");
    py::array_t<int64_t> out({(py::ssize_t)N});
    flood_wide((const uint8_t *)k.data(), sigma, N, out.mutable_data());
    return out;
  }, py::arg("fkey"), py::arg("smudge_bits"), py::arg("N"));
  mseal.def("_decrypt_share_host", [](uint32_t N, const std::vector<uint64_t> &primes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> s_ntt,
                                      py::array_t<uint64_t, py::array::c_style | py::array::forcecast> ct, uint32_t sigma, py::bytes fk) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    const std::string k = fk;
    if (k.size() != 32) throw std::invalid_argument("a flooding key is 32 bytes");
    if (ct.ndim() != 3) throw std::invalid_argument("ciphertext words are [size][limbs][N]");
    SecretKey sk;
    sk.s_ntt.assign((const u64 *)s_ntt.data(), (const u64 *)s_ntt.data() + s_ntt.size());
    HostCipher c;
    c.size = (uint32_t)ct.shape(0);
    c.limbs = (uint32_t)ct.shape(1);
    c.data.assign((const u64 *)ct.data(), (const u64 *)ct.data() + ct.size());
    std::array<uint8_t, 32> key;
    std::memcpy(key.data(), k.data(), 32);
    return to_numpy(decrypt_share_host(h, sk, c, sigma, key), {(py::ssize_t)c.limbs, (py::ssize_t)N});
  }, py::arg("N"), py::arg("primes"), py::arg("s_ntt"), py::arg("ct"), py::arg("smudge_bits"), py::arg("fkey"));
  mseal.def("_combine_shares_host", [](uint32_t N, const std::vector<uint64_t> &primes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> ct,
                                       py::array_t<uint64_t, py::array::c_style | py::array::forcecast> shares, uint32_t sigma, double scale) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    if (ct.ndim() != 3) throw std::invalid_argument("ciphertext words are [size][limbs][N]");
    HostCipher c;
    c.size = (uint32_t)ct.shape(0);
    c.limbs = (uint32_t)ct.shape(1);
    c.scale = scale;
    c.data.assign((const u64 *)ct.data(), (const u64 *)ct.data() + ct.size());
    if (shares.ndim() != 3 || shares.shape(1) != (py::ssize_t)c.limbs || shares.shape(2) != (py::ssize_t)N)
      throw std::invalid_argument("shares are [parties][limbs][N]");
    std::vector<const u64 *> hs;
    for (py::ssize_t p = 0; p < shares.shape(0); p++) hs.push_back((const u64 *)shares.data() + (size_t)p * c.limbs * N);
    const std::vector<u64> m = combine_shares_host(h, c, hs, sigma);
    std::vector<double> v;
    h.decode_coeff(m.data(), c.limbs, scale, v);
    py::array_t<double> vals({(py::ssize_t)v.size()});
    std::memcpy(vals.mutable_data(), v.data(), v.size() * sizeof(double));
    return py::make_tuple(to_numpy(m, {(py::ssize_t)c.limbs, (py::ssize_t)N}), vals);
  }, py::arg("N"), py::arg("primes"), py::arg("ct"), py::arg("shares"), py::arg("smudge_bits"), py::arg("scale"));
  // test hook: the host twin of evah_keygen_rekey (ckks_host.h rekey_keygen_host) on raw words -> [digits][2][k][N]
  mseal.def("_rekey_keygen_host", [](uint32_t N, const std::vector<uint64_t> &primes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> s_ntt,
                                     py::array_t<uint64_t, py::array::c_style | py::array::forcecast> pk,
                                     py::array_t<uint8_t, py::array::c_style | py::array::forcecast> rkeys) {
    HostContext h(N, std::vector<u64>(primes.begin(), primes.end()));
    if (rkeys.ndim() != 2 || rkeys.shape(1) != 32) throw std::invalid_argument("randomness keys are [digits][32] bytes");
    SecretKey sk;
    sk.s_ntt.assign((const u64 *)s_ntt.data(), (const u64 *)s_ntt.data() + s_ntt.size());
    PublicKey pkt;
    pkt.data.assign((const u64 *)pk.data(), (const u64 *)pk.data() + pk.size());
    const uint32_t D = (uint32_t)rkeys.shape(0);
    std::vector<std::array<uint8_t, 32>> rk(D);
    for (uint32_t J = 0; J < D; J++) std::memcpy(rk[J].data(), rkeys.data() + (size_t)32 * J, 32);
    return to_numpy(rekey_keygen_host(h, sk, pkt, D, rk.data()), {(py::ssize_t)D, 2, (py::ssize_t)h.k, (py::ssize_t)N});
  }, py::arg("N"), py::arg("primes"), py::arg("s_ntt"), py::arg("pk"), py::arg("rkeys"));
  py::class_<DecryptionShares, std::shared_ptr<DecryptionShares>>(mseal, "DecryptionShares",
                                                                  "One party's contribution to the joint opening of a valuation (DESIGN.md 1.14): made by "
                                                                  "SEALSecret.decrypt_share, combined by SEALPublic.combine_shares; saves and loads")
      .def_readonly("poly_modulus_degree", &DecryptionShares::N)
      .def_readonly("primes", &DecryptionShares::primes)
      .def_readonly("smudge_bits", &DecryptionShares::smudge_bits)
      .def_readonly("batch", &DecryptionShares::batch)
      .def_readonly("B", &DecryptionShares::B)
      .def("names", [](const DecryptionShares &d) {
        std::vector<std::string> n;
        for (auto &kv : d.values) n.push_back(kv.first);
        return n;
      })
      .def("words", [](const DecryptionShares &d, const std::string &name) {
        auto it = d.values.find(name);
        if (it == d.values.end()) throw py::key_error(name);
        py::list out; // one array [n][limbs][N] per piece (a resident piece is downloaded)
        for (const SharePiece &p : it->second)
          out.append(to_numpy(words(p, d.N), {(py::ssize_t)p.n, (py::ssize_t)p.limbs, (py::ssize_t)d.N}));
        return out;
      }, py::arg("name"), "the share of `name` as host words: a list of arrays [instances][limbs][N], one per device call");
  py::class_<RekeyKey, std::shared_ptr<RekeyKey>>(mseal, "RekeyKey",
                                                  "The key that takes results under one key pair to another of the same parameters (DESIGN.md 1.13): made by "
                                                  "SEALSecret.make_rekey_key from the target's public context, applied by the target's SEALPublic.rekey")
      .def_readonly("poly_modulus_degree", &RekeyKey::N)
      .def_readonly("primes", &RekeyKey::primes)
      .def_readonly("n_digits", &RekeyKey::n_digits)
      .def("words", [](const RekeyKey &k) {
        return to_numpy(k.data, {(py::ssize_t)k.n_digits, 2, (py::ssize_t)k.primes.size(), (py::ssize_t)k.N});
      }, "the key [digits][2][k][N], NTT form");
  py::class_<HipValuation>(mseal, "SEALValuation", "Inputs or outputs of execute(): ciphertexts, plaintexts or raw vectors")
      .def(py::init<>())
      .def("_set_cipher", [](HipValuation &v, const std::string &name, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> data, double scale) {
        if (data.ndim() != 3) throw std::invalid_argument("cipher data must be [size][limbs][N]");
        HostCipher c;
        c.size = (uint32_t)data.shape(0);
        c.limbs = (uint32_t)data.shape(1);
        c.scale = scale;
        c.data.assign((const u64 *)data.data(), (const u64 *)data.data() + data.size());
        v.values[name] = std::move(c);
      })
      .def("_set_plain", [](HipValuation &v, const std::string &name, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> data, double scale) {
        if (data.ndim() != 2) throw std::invalid_argument("plain data must be [limbs][N]");
        HostPlain p;
        p.limbs = (uint32_t)data.shape(0);
        p.scale = scale;
        p.data.assign((const u64 *)data.data(), (const u64 *)data.data() + data.size());
        v.values[name] = std::move(p);
      })
      .def("_set_raw", [](HipValuation &v, const std::string &name, std::vector<double> data) { v.values[name] = std::move(data); })
      // a valuation assembled by hand or loaded from this repo's container carries no encryption parameters; the SEAL
      // wire format needs them (SEALValuation::params, seal.h:23-27)
      .def("_set_params", [](HipValuation &v, const HipPublic &p) { v.params = p.host; }, py::arg("public_ctx"))
      .def("names", [](const HipValuation &v) { std::vector<std::string> n; for (auto &kv : v.values) n.push_back(kv.first); return n; })
      .def("is_resident", [](const HipValuation &v, const std::string &name) {
        auto it = v.values.find(name);
        if (it == v.values.end()) throw std::out_of_range("No value named " + name);
        auto *c = std::get_if<HostCipher>(&it->second);
        return c && c->dev != nullptr;
      }, py::arg("name"), "True while the ciphertext lives in HBM (a handle of the device context that produced it)")
      .def("on_host", [](const HipValuation &v, const std::string &name) {
        auto it = v.values.find(name);
        if (it == v.values.end()) throw std::out_of_range("No value named " + name);
        auto *c = std::get_if<HostCipher>(&it->second);
        return !c || !c->data.empty() || seeded_on_host(*c);
      }, py::arg("name"), "True when host words of the value exist (always, for plaintexts and raw vectors; c0 + seed for a seeded ciphertext)")
      .def("seed", [](const HipValuation &v, const std::string &name) -> py::object {
        auto it = v.values.find(name);
        if (it == v.values.end()) throw std::out_of_range("No value named " + name);
        auto *c = std::get_if<HostCipher>(&it->second);
        if (!c || !c->seeded) return py::none();
        return py::bytes(reinterpret_cast<const char *>(c->seeded->seed.data()), 32);
      }, py::arg("name"), "The 32-byte seed of c1 of a ciphertext from SEALSecret.encrypt (DESIGN.md 1.3), else None")
      .def("to_host", [](HipValuation &v, bool drop_device) {
        for (auto &kv : v.values)
          if (auto *c = std::get_if<HostCipher>(&kv.second)) {
            (void)words(*c);
            if (drop_device) c->dev.reset();
          }
      }, py::arg("drop_device") = false, "Download every device-resident ciphertext (waits for it); drop_device releases the HBM copies")
      // (kind, size, limbs, scale, data) — raw residues for the bit-exact parity tests
      .def("get", [](const HipValuation &v, const std::string &name) -> py::object {
        auto it = v.values.find(name);
        if (it == v.values.end()) throw std::out_of_range("No value named " + name);
        if (auto *c = std::get_if<HostCipher>(&it->second)) {
          const CipherWords &w = words(*c); // a device-resident value is downloaded (and kept) here
          py::ssize_t n = (py::ssize_t)(w.size() / ((size_t)c->size * c->limbs));
          return py::make_tuple("cipher", c->size, c->limbs, c->scale, to_numpy(w, {(py::ssize_t)c->size, (py::ssize_t)c->limbs, n}));
        }
        if (auto *p = std::get_if<HostPlain>(&it->second)) {
          py::ssize_t n = (py::ssize_t)(p->data.size() / p->limbs);
          return py::make_tuple("plain", 1, p->limbs, p->scale, to_numpy(p->data, {(py::ssize_t)p->limbs, n}));
        }
        return py::make_tuple("raw", 0, 0, 1.0, py::cast(std::get<std::vector<double>>(it->second)));
      });
  py::class_<HipValuationBatch>(mseal, "SEALValuationBatch",
                                "B valuations of one shape as batched device handles (DESIGN.md 1.9): what encrypt_array returns, "
                                "execute_batch takes and returns, and decrypt_array reads")
      .def("__len__", [](const HipValuationBatch &v) { return v.B; })
      .def("names", [](const HipValuationBatch &v) {
        std::vector<std::string> n;
        for (auto &kv : v.ciphers) n.push_back(kv.first);
        for (auto &kv : v.shared) n.push_back(kv.first);
        for (auto &kv : v.plains) n.push_back(kv.first);
        return n;
      })
      .def("plain_arrays", [](const HipValuationBatch &v) {
        py::dict d;
        for (auto &kv : v.plains) {
          const ArrayView &a = kv.second.view;
          const py::dtype dt = a.dtype == EVAH_F64 ? py::dtype::of<double>() : a.dtype == EVAH_F32 ? py::dtype::of<float>() : py::dtype::of<uint8_t>();
          py::array arr(dt, std::vector<py::ssize_t>{(py::ssize_t)a.B, (py::ssize_t)a.n});
          std::memcpy(arr.mutable_data(), a.data, a.B * a.n * a.itemsize());
          d[py::str(kv.first)] = arr;
        }
        return d;
      }, "the unencrypted values that differ per instance (DESIGN.md 1.10): {name: ndarray [B, n]} in the type they are held in")
      .def("segments", [](const HipValuationBatch &v, const std::string &name) {
        auto it = v.ciphers.find(name);
        if (it == v.ciphers.end()) throw std::out_of_range("No encrypted value named " + name);
        std::vector<uint32_t> n;
        for (auto &s : it->second.segments) n.push_back(s.n);
        return n;
      }, py::arg("name"), "instances per batched handle of an encrypted value, in instance order")
      .def("__getitem__", [](const HipValuationBatch &v, py::ssize_t b) {
        if (b < 0) b += (py::ssize_t)v.B;
        if (b < 0 || (size_t)b >= v.B) throw py::index_error("instance index out of range");
        return batch_instance(v, (size_t)b);
      }, "instance b as a SEALValuation whose ciphertexts are views of the batched handles")
      .def("to_list", [](const HipValuationBatch &v) {
        std::vector<HipValuation> out;
        for (size_t b = 0; b < v.B; b++) out.push_back(batch_instance(v, b));
        return out;
      }, "every instance as a SEALValuation (views; a symmetric value keeps its seed, so save() still writes it compressed)");
  py::class_<HipPublic, std::shared_ptr<HipPublic>>(mseal, "SEALPublic", "Public context: encryption and execution on the MI355X")
      .def("_encrypt_array", [](HipPublic &p, const std::map<std::string, py::array> &arrays, const Valuation &shared, const CKKSSignature &sig,
                                uint64_t seed, const std::map<std::string, py::array> &plains, const DevArrayArgs &dev_arrays) {
             return p.encrypt_array(with_device_arrays(array_views(arrays), dev_arrays), shared, sig, seed, array_views(plains));
           },
           py::arg("arrays"), py::arg("shared"), py::arg("signature"), py::arg("seed") = 0, py::arg("plain_arrays") = std::map<std::string, py::array>{},
           py::arg("device_arrays") = DevArrayArgs{},
           "encrypt_array on normalised arguments (eva_amd.seal.normalise_arrays): C-contiguous [B, n] arrays of float64, float32 or uint8; "
           "device_arrays: rows in device memory (eva_amd.seal.normalise_device_arrays)")
      .def("execute_batch", [](HipPublic &p, Program &program, const HipValuationBatch &inputs) { return p.execute_batch(program, inputs); },
           py::arg("program"), py::arg("inputs"),
           "execute_batch on a SEALValuationBatch: each group's inputs are slices of the batch's handles and its batched outputs are the "
           "segments of the returned SEALValuationBatch; nothing is stacked, unstacked or copied. In the multi-device modes (devices or shard "
           "set) the call goes through to_list() and the list path")
      .def("stack_stats", [](HipPublic &p) {
        auto st = p.stack_stats();
        py::dict d;
        d["calls"] = st[0]; d["instances"] = st[1];
        return d;
      }, "evah_ct_stack calls on the context's device state so far and the instances they copied")
      .def("encrypt", [](HipPublic &p, const Valuation &inputs, const CKKSSignature &sig) {
        HipValuation v = p.encrypt(inputs, sig);
        v.params = p.host;
        return v;
      }, py::arg("inputs"), py::arg("signature"))
      .def("encrypt_batch", [](HipPublic &p, const std::vector<Valuation> &inputs, const CKKSSignature &sig, bool device_sampling, uint64_t seed) {
        std::vector<HipValuation> out = p.encrypt_batch(inputs, sig, device_sampling, seed);
        for (HipValuation &v : out) v.params = p.host;
        return out;
      }, py::arg("inputs"), py::arg("signature"), py::arg("device_sampling") = false, py::arg("seed") = 0,
           "encrypt() for a list of input valuations with the same input names; per name the instances are encoded and encrypted 64 at a time in one device call. "
           "device_sampling: each encrypted input's u, e0, e1 are expanded from a 32-byte randomness key, on the device in the grouped calls "
           "(DESIGN.md 1.7); seed != 0 (with device_sampling only): reproducible test stream, not secret-grade")
      // test hook: the host encoder + the host encryptor on the caller's randomness, small = int8 [3][N] = (u, e0, e1)
      .def("_encrypt_with", [](const HipPublic &p, const std::vector<double> &values, uint32_t scale_bits, uint32_t level,
                               py::array_t<int8_t, py::array::c_style | py::array::forcecast> small) {
        const HostContext &h = *p.host;
        const size_t slots = h.N / 2, N = h.N;
        if (values.empty() || slots % values.size()) throw std::runtime_error("Size must exactly divide slots");
        if (level >= h.k - 1) throw std::runtime_error("Encode level exceeds the modulus chain");
        if (small.ndim() != 2 || small.shape(0) != 3 || small.shape(1) != (py::ssize_t)N) throw std::invalid_argument("small must be int8 [3][N]");
        HostPlain pt;
        pt.limbs = h.k - 1 - level;
        pt.scale = std::pow(2.0, (double)scale_bits);
        pt.data.resize((size_t)pt.limbs * N);
        std::vector<double> vec;
        for (size_t r = slots / values.size(); r > 0; --r) vec.insert(vec.end(), values.begin(), values.end());
        h.encode_coeff(vec.data(), pt.scale, pt.limbs, pt.data.data());
        for (uint32_t i = 0; i < pt.limbs; i++) h.ntt(i, pt.data.data() + (size_t)i * N);
        const int8_t *d = small.data();
        const HostCipher c = evahost::encrypt(h, p.pk, pt, std::vector<int8_t>(d, d + N), std::vector<int8_t>(d + N, d + 2 * N),
                                              std::vector<int8_t>(d + 2 * N, d + 3 * N));
        return to_numpy(c.data, {2, (py::ssize_t)c.limbs, (py::ssize_t)N});
      }, py::arg("values"), py::arg("scale_bits"), py::arg("level"), py::arg("small"))
      .def("execute", [](HipPublic &p, Program &program, const HipValuation &inputs) {
        HipValuation v = p.execute(program, inputs);
        v.params = p.host;
        return v;
      }, py::arg("program"), py::arg("inputs"))
      .def("execute_batch", [](HipPublic &p, Program &program, const std::vector<const HipValuation *> &inputs) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<HipValuation> out = p.execute_batch(program, inputs);
        for (HipValuation &v : out) v.params = p.host;
        if (std::getenv("EVA_BATCH_TIMING"))
          std::fprintf(stderr, "EVA: execute_batch binding: %.3f ms inside (before the results become Python objects)\n",
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return out;
      }, py::arg("program"), py::arg("inputs"),
           "execute() for a list of independent input valuations of one program; instances run batch_chunk at a time as batched device handles")
      .def_readwrite("library_scheduler", &HipPublic::library_scheduler, "run the encrypted part of a program as one evah_execute (default) instead of the node-by-node host walk")
      .def_readwrite("batch_chunk", &HipPublic::batch_chunk, "instances per batched device handle in execute_batch (1..64)")
      .def_readwrite("batch_ramp", &HipPublic::batch_ramp, "execute_batch: quarter / three-quarter sized groups at both ends of the batch, so the pipeline fills and drains on small copies (EVA_BATCH_RAMP)")
      .def_readwrite("batch_balance", &HipPublic::batch_balance, "execute_batch: groups of (nearly) equal size instead of full groups and a remainder (EVA_BATCH_BALANCE)")
      .def_readwrite("batch_depth", &HipPublic::batch_depth, "groups in flight in execute_batch = issue queues it rotates over (2..8; 0 = three on resident valuations, four on host valuations; EVA_BATCH_DEPTH)")
      .def_readwrite("device", &HipPublic::device)
      .def_readwrite("free_eagerly", &HipPublic::free_eagerly)
      .def_readwrite("use_graphs", &HipPublic::use_graphs, "replay repeated executions of one program from a captured hipGraph")
      .def("_graph_plans", [](HipPublic &p) { return p.graph_plan_count(); }, "captured plans alive (a program found busy by the next call has two)")
      .def_readwrite("twin_plans", &HipPublic::twin_plans, "a program whose replay is found busy by the next execute() gets a second captured plan on its own queue; calls then go to whichever is idle (EVA_GRAPH_TWIN)")
      .def("drop_graphs", &HipPublic::drop_graphs)
      .def_readwrite("devices", &HipPublic::devices, "device index per member of the multi-GPU modes (a repeated index = several contexts on one GPU)")
      .def_readwrite("shard_mode", &HipPublic::shard_mode, "'' (one device) | 'subdag' | 'limb' | 'dag' — how execute() / execute_batch() use `devices`")
      .def_readonly("last_subdag_plan", &HipPublic::last_subdag_plan, "(member, ops) per piece of the last sub-DAG split: prefix, components..., suffix")
      .def("key_upload_stats", [](HipPublic &p) {
        auto st = p.key_upload_stats();
        py::dict d;
        d["uploads"] = st[0]; d["bytes"] = st[1];
        return d;
      }, "evaluation keys uploaded from the host to the context's own device so far: calls and bytes sent (keys generated on the device count in neither)")
      .def("key_host_bytes", &HipPublic::key_host_bytes, "bytes of evaluation-key words held on the host right now: 0 while keys generated in place keep their c0 on the device only (DESIGN.md 1.8)")
      .def("key_bytes", &HipPublic::key_bytes, "HBM bytes of evaluation keys: one entry per limb shard (when limb-sharded), then the whole keys on the context's own device (0 if never uploaded)")
      .def("set_limb_dist", [](HipPublic &p, uint32_t rank, uint32_t world, py::object all_gather, py::object broadcast, py::object sum_host,
                               uintptr_t stream) {
        // the exchange steps of limb sharding across processes, as callbacks into torch.distributed (RCCL); called
        // from execute() with the GIL held
        p.limb_rank = rank;
        p.limb_world = world;
        p.limb_stream = stream;
        p.limb_hooks.all_gather = [all_gather](void *ptr, size_t chunk) { all_gather((uintptr_t)ptr, chunk); };
        p.limb_hooks.broadcast = [broadcast](void *ptr, size_t words, uint32_t owner) { broadcast((uintptr_t)ptr, words, owner); };
        p.limb_hooks.sum_host = [sum_host](evahost::u64 *w, size_t n) {
          sum_host(py::array_t<uint64_t>({(py::ssize_t)n}, {(py::ssize_t)sizeof(uint64_t)}, (const uint64_t *)w, py::capsule(w, [](void *) {})));
        };
        p.shard_mode = "limb";
      }, py::arg("rank"), py::arg("world"), py::arg("all_gather"), py::arg("broadcast"), py::arg("sum_host"), py::arg("stream") = 0,
           "limb sharding across processes: this context is shard `rank` of `world`; all_gather(ptr, chunk_words), "
           "broadcast(ptr, words, owner) act in place on device buffers, sum_host(array) all-reduces a host uint64 array")
      .def_readonly("last_exchanged_words", &HipPublic::last_exchanged_words, "uint64 words moved between shards by the last limb-sharded execute()")
      .def_readonly("last_exchange_launches", &HipPublic::last_exchange_launches,
                    "launches those words took: one per receiving shard per exchange step (evah_buf_gather)")
      .def_readwrite("resident", &HipPublic::resident, "keep valuations in HBM: encrypt/execute return device handles and execute does not wait for the GPU (EVA_RESIDENT=0: host valuations)")
      .def_readwrite("graph_copy_limit", &HipPublic::graph_copy_limit, "device-resident inputs above this many bytes are walked eagerly instead of copied into a captured graph's slots")
      .def("synchronize", &HipPublic::synchronize, "wait for everything this context has enqueued")
      .def("combine_shares", [](HipPublic &p, py::object enc, const std::vector<std::shared_ptr<DecryptionShares>> &shares, const CKKSSignature &sig,
                                py::object dtype, bool device) -> py::object {
        if (!py::isinstance<HipValuationBatch>(enc)) return py::cast(p.combine_shares(enc.cast<const HipValuation &>(), shares, sig));
        const HipValuationBatch &vb = enc.cast<const HipValuationBatch &>();
        const py::dtype dt = py::dtype::from_args(dtype);
        int code;
        if (dt.kind() == 'f' && dt.itemsize() == 8) code = EVAH_F64;
        else if (dt.kind() == 'f' && dt.itemsize() == 4) code = EVAH_F32;
        else if (dt.kind() == 'u' && dt.itemsize() == 1) code = EVAH_U8;
        else throw std::invalid_argument("combine_shares: dtype must be float64, float32 or uint8");
        if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
        py::dict out;
        std::map<std::string, void *> rows;
        for (auto &kv : vb.ciphers) {
          if (device) {
            auto a = std::make_shared<DeviceArray>(p.device_state(), code, vb.B, (size_t)sig.vec_size);
            rows[kv.first] = a->ptr();
            out[py::str(kv.first)] = a;
          } else {
            py::array a(dt, std::vector<py::ssize_t>{(py::ssize_t)vb.B, (py::ssize_t)sig.vec_size});
            rows[kv.first] = a.mutable_data();
            out[py::str(kv.first)] = a;
          }
        }
        p.combine_shares_array(vb, shares, sig, code, rows, device);
        for (auto &kv : vb.shared) { // one value for all instances, as decrypt_array returns it
          if (std::holds_alternative<HostCipher>(kv.second)) continue;
          const std::vector<double> v = decode_unencrypted(*p.host, kv.second, (size_t)sig.vec_size);
          py::array_t<double> a({(py::ssize_t)vb.B, (py::ssize_t)sig.vec_size});
          for (size_t b = 0; b < vb.B; b++) std::copy(v.begin(), v.end(), a.mutable_data() + b * v.size());
          out[py::str(kv.first)] = code == EVAH_U8 ? as_uint8(a) : code == EVAH_F32 ? py::array(a.attr("astype")(dt)) : py::array(a);
        }
        return out;
      }, py::arg("enc"), py::arg("shares"), py::arg("signature"), py::arg("dtype") = py::module_::import("numpy").attr("float64"), py::arg("device") = false,
           "Open a valuation from the decryption shares of EVERY party of a collective key (DESIGN.md 1.14): m = c0 + the sum of the shares, "
           "then decrypt()'s decoder. Needs no secret key. enc: a SEALValuation (returns what decrypt returns) or a SEALValuationBatch (returns what "
           "decrypt_array returns, dtype and device as there); shares: one DecryptionShares per party, made from this enc with one smudge_bits. "
           "A slot differs from the decryption under the whole key by at most N * P * 2^smudge_bits / scale")
      .def("install_rekey_key", [](HipPublic &p, std::shared_ptr<RekeyKey> rk) { return p.install_rekey_key(rk); }, py::arg("rekey_key"),
           "upload a RekeyKey to this context's device state (once per key); returns its slot")
      .def("rekey", [](HipPublic &p, py::object enc, std::shared_ptr<RekeyKey> rk) -> py::object {
        if (py::isinstance<HipValuationBatch>(enc)) return py::cast(p.rekey_batch(enc.cast<const HipValuationBatch &>(), rk));
        return py::cast(p.rekey(enc.cast<const HipValuation &>(), rk));
      }, py::arg("enc"), py::arg("rekey_key"),
           "Re-key (DESIGN.md 1.13): the encrypted values of a SEALValuation or SEALValuationBatch under another key pair become values under "
           "this one, with the RekeyKey that pair's secret context made from this public context; level and scale stay, the results are "
           "resident on this context's device state, unencrypted and raw values pass through. Size-2 ciphertexts only (relinearize first). "
           "A value on this GPU is read in place; no secret key is involved")
      .def("transfer_stats", [](HipPublic &p) {
        auto st = p.transfer_stats();
        py::dict d;
        d["ct_uploads"] = st[0]; d["ct_downloads"] = st[1]; d["pt_uploads"] = st[2]; d["pt_downloads"] = st[3];
        d["h2d_bytes"] = st[4]; d["d2h_bytes"] = st[5];
        return d;
      }, "ciphertext / plaintext transfers across the host boundary since the device context was created")
      .def("profile", &HipPublic::profile, py::arg("on"), "HIP-event brackets around every kernel launch of this context's issue queues, by kernel class")
      .def("profile_reset", &HipPublic::profile_reset)
      .def("profile_get", [](HipPublic &p) {
        py::dict d;
        for (auto &kv : p.profile_get()) d[py::str(kv.first)] = py::make_tuple(kv.second.first, kv.second.second);
        return d;
      }, "{kernel class: (launches, total ms)} since the last profile_reset(), summed over the issue queues")
      .def_readonly("last_timing", &HipPublic::last_timing, "ms of the last execute(): (input upload, DAG enqueue on the host, drain + output download)")
      .def_readwrite("num_queues", &HipPublic::num_queues, "HIP streams independent DAG nodes are spread over")
      .def_property_readonly("poly_modulus_degree", [](const HipPublic &p) { return p.host->N; })
      .def_property_readonly("primes", [](const HipPublic &p) { return std::vector<uint64_t>(p.host->primes.begin(), p.host->primes.end()); })
      .def_readonly("dropped_galois_elements", &HipPublic::dropped_galois,
                    "combine_public_contexts: the Galois elements that some party's context lacked and this collective context therefore has no key for")
      .def_readonly("collective", &HipPublic::collective, "made by combine_public_contexts (DESIGN.md 1.14); see has_relin_key")
      .def_property_readonly("has_relin_key", &HipPublic::has_relin_key,
                             "False only for a collective context whose parties did not run the relinearization-key rounds (DESIGN.md 1.15)")
      // host FP64 encoder + host NTT: the plaintext an Encode node produces (tests pin the
      // integer path "from the encoded plaintext onward")
      .def("_encode", [](const HipPublic &p, const std::vector<double> &values, uint32_t scale_bits, uint32_t level) {
        const HostContext &h = *p.host;
        const size_t slots = h.N / 2;
        if (values.empty() || slots % values.size()) throw std::runtime_error("Size must exactly divide slots");
        if (level >= h.k - 1) throw std::runtime_error("Encode level exceeds the modulus chain");
        const uint32_t limbs = h.k - 1 - level;
        std::vector<double> vec;
        for (size_t r = slots / values.size(); r > 0; --r) vec.insert(vec.end(), values.begin(), values.end());
        std::vector<u64> out((size_t)limbs * h.N);
        h.encode_coeff(vec.data(), std::pow(2.0, (double)scale_bits), limbs, out.data());
        for (uint32_t i = 0; i < limbs; i++) h.ntt(i, out.data() + (size_t)i * h.N);
        return to_numpy(out, {(py::ssize_t)limbs, (py::ssize_t)h.N});
      }, py::arg("values"), py::arg("scale_bits"), py::arg("level"))
      // the full words of a key, materialised for the caller when the context keeps it compressed (which it goes on doing)
      .def("relin_key", [](const HipPublic &p) {
        if (!p.has_relin_key()) throw std::invalid_argument(p.no_relin_key_message());
        std::vector<u64> tmp;
        return to_numpy(p.relin.words(*p.host, tmp), {(py::ssize_t)p.relin.n_digits, 2, (py::ssize_t)p.host->k, (py::ssize_t)p.host->N});
      })
      .def_property_readonly("keys_compressed", &HipPublic::keys_compressed, "the evaluation keys are kept, saved and uploaded as c0 + a 32-byte seed per digit (generate_keys(..., compress_keys=True)). "
                             "For a collective context this speaks of the Galois keys: its relinearization key, if it has one, is kept whole")
      .def("key_seeds", [](const HipPublic &p) -> py::object {
        if (!p.keys_compressed()) return py::none();
        auto seeds_of = [](const SwitchKey &k) {
          py::array_t<uint8_t> a({(py::ssize_t)k.n_digits, (py::ssize_t)32});
          std::memcpy(a.mutable_data(), k.seeds.data(), k.seeds.size());
          return a;
        };
        py::dict d;
        if (p.relin.compressed()) d[py::int_(0)] = seeds_of(p.relin); // a collective context's key is whole: no entry
        for (auto &kv : p.galois) d[py::int_(kv.first)] = seeds_of(kv.second);
        return d;
      }, "{0: the relinearization key's seeds [digits][32], Galois element: that key's} of a compressed context (DESIGN.md 1.4), else None; "
         "a key that is kept whole (the relinearization key of a collective context) has no entry")
      .def("public_key", [](const HipPublic &p) { return to_numpy(p.pk.data, {2, (py::ssize_t)p.host->k, (py::ssize_t)p.host->N}); })
      .def("galois_keys", [](const HipPublic &p) {
        py::dict d;
        std::vector<u64> tmp;
        for (auto &kv : p.galois)
          d[py::int_(kv.first)] = to_numpy(kv.second.words(*p.host, tmp), {(py::ssize_t)kv.second.n_digits, 2, (py::ssize_t)p.host->k, (py::ssize_t)p.host->N});
        return d;
      });
  py::class_<DeviceArray, std::shared_ptr<DeviceArray>>(mseal, "DeviceArray",
                                                        "decrypted rows [B, vec_size] in the key pair's device state (decrypt_array(device=True), DESIGN.md 1.11); "
                                                        "the memory is zeroed on the queue before it returns to the pool")
      .def_property_readonly("shape", [](const DeviceArray &a) { return py::make_tuple(a.B, a.n); })
      .def_property_readonly("dtype", [](const DeviceArray &a) {
        return py::dtype(a.dtype == EVAH_F64 ? "float64" : a.dtype == EVAH_F32 ? "float32" : "uint8");
      })
      .def_property_readonly("ptr", [](const DeviceArray &a) { return (uintptr_t)a.ptr(); })
      .def_property_readonly("__cuda_array_interface__", [](const DeviceArray &a) {
        py::dict d;
        d["shape"] = py::make_tuple(a.B, a.n);
        d["typestr"] = a.dtype == EVAH_F64 ? "<f8" : a.dtype == EVAH_F32 ? "<f4" : "|u1";
        d["data"] = py::make_tuple((uintptr_t)a.ptr(), false);
        d["strides"] = py::none();
        d["version"] = 3;
        return d;
      })
      .def("to_numpy", [](const DeviceArray &a) {
        const size_t words = (a.bytes() + 7) / 8;
        std::vector<uint64_t> w(words);
        chk(evah_buf_download(a.dev->h, a.buf, 0, words, w.data()));
        py::array out(py::dtype(a.dtype == EVAH_F64 ? "float64" : a.dtype == EVAH_F32 ? "float32" : "uint8"),
                      std::vector<py::ssize_t>{(py::ssize_t)a.B, (py::ssize_t)a.n});
        std::memcpy(out.mutable_data(), w.data(), a.bytes());
        return out;
      }, "the rows on the host (a synchronising download)");
  py::class_<HipSecret, std::shared_ptr<HipSecret>>(mseal, "SEALSecret", "Secret context: decryption. Holds the secret key.")
      .def("encrypt", [](HipSecret &s, const Valuation &inputs, const CKKSSignature &sig, uint64_t seed) {
        HipValuation v = s.encrypt(inputs, sig, seed);
        v.params = s.host;
        return v;
      }, py::arg("inputs"), py::arg("signature"), py::arg("seed") = 0,
         "Secret-key encryption: every ciphertext is c0 plus the 32-byte seed of c1 (half the bytes of SEALPublic.encrypt). "
         "seed != 0: reproducible test streams, not secret-grade")
      .def("encrypt_batch", [](HipSecret &s, const std::vector<Valuation> &inputs, const CKKSSignature &sig, uint64_t seed, bool device_sampling) {
        std::vector<HipValuation> out = s.encrypt_batch(inputs, sig, seed, device_sampling);
        for (HipValuation &v : out) v.params = s.host;
        return out;
      }, py::arg("inputs"), py::arg("signature"), py::arg("seed") = 0, py::arg("device_sampling") = false,
         "encrypt() for a list of input valuations with the same input names: one pair of random streams for the call, instances in list "
         "order and names sorted within an instance, so instance 0 of a seeded call equals encrypt() and no two values share a seed. "
         "device_sampling: each error polynomial is expanded from a 32-byte key of the secret stream, on the device in the grouped calls (DESIGN.md 1.7)")
      .def("_encrypt_array", [](HipSecret &s, const std::map<std::string, py::array> &arrays, const Valuation &shared, const CKKSSignature &sig,
                                uint64_t seed, const std::map<std::string, py::array> &plains, const DevArrayArgs &dev_arrays) {
             return s.encrypt_array(with_device_arrays(array_views(arrays), dev_arrays), shared, sig, seed, array_views(plains));
           },
           py::arg("arrays"), py::arg("shared"), py::arg("signature"), py::arg("seed") = 0, py::arg("plain_arrays") = std::map<std::string, py::array>{},
           py::arg("device_arrays") = DevArrayArgs{},
           "encrypt_array on normalised arguments (eva_amd.seal.normalise_arrays); every ciphertext is seeded")
      .def("decrypt_array", [](HipSecret &s, py::object enc, const CKKSSignature &sig, py::object dtype, bool device) {
        const py::dtype dt = py::dtype::from_args(dtype);
        int code;
        if (dt.kind() == 'f' && dt.itemsize() == 8) code = EVAH_F64;
        else if (dt.kind() == 'f' && dt.itemsize() == 4) code = EVAH_F32;
        else if (dt.kind() == 'u' && dt.itemsize() == 1) code = EVAH_U8;
        else throw std::invalid_argument("decrypt_array: dtype must be float64, float32 or uint8");
        if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
        HipValuationBatch from_list;
        const HipValuationBatch *vb;
        if (py::isinstance<HipValuationBatch>(enc)) {
          vb = &enc.cast<const HipValuationBatch &>();
        } else {
          if (!s.on_device()) throw std::runtime_error("decrypt_array needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
          from_list = batch_of_list(enc.cast<std::vector<const HipValuation *>>(), s.dev, s.host);
          vb = &from_list;
        }
        py::dict out;
        std::map<std::string, void *> rows;
        if (device) { // the rows stay in the key pair's device state; unencrypted outputs below stay numpy arrays
          if (!s.on_device()) throw std::runtime_error("decrypt_array needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
          for (auto &kv : vb->ciphers) {
            auto a = std::make_shared<DeviceArray>(s.dev, code, vb->B, (size_t)sig.vec_size);
            rows[kv.first] = a->ptr();
            out[py::str(kv.first)] = a;
          }
        } else {
          for (auto &kv : vb->ciphers) {
            py::array a(dt, std::vector<py::ssize_t>{(py::ssize_t)vb->B, (py::ssize_t)sig.vec_size});
            rows[kv.first] = a.mutable_data();
            out[py::str(kv.first)] = a;
          }
        }
        s.decrypt_array(*vb, sig, code, rows, device);
        for (auto &kv : vb->shared) { // one value for all instances: decrypt()'s doubles in every row
          const std::vector<double> v = s.decrypt_value(kv.first, kv.second, sig);
          py::array_t<double> a({(py::ssize_t)vb->B, (py::ssize_t)sig.vec_size});
          for (size_t b = 0; b < vb->B; b++) std::copy(v.begin(), v.end(), a.mutable_data() + b * v.size());
          out[py::str(kv.first)] = code == EVAH_U8 ? as_uint8(a) : code == EVAH_F32 ? py::array(a.attr("astype")(dt)) : py::array(a);
        }
        for (auto &kv : vb->plains) { // an unencrypted output with a row per instance: [B, vec_size] float64
          const ArrayView &pv = kv.second.view;
          if (pv.n < 1 || (size_t)sig.vec_size % pv.n) throw std::runtime_error("Output " + kv.first + " does not match the signature's vector size");
          py::array_t<double> a({(py::ssize_t)vb->B, (py::ssize_t)sig.vec_size});
          for (size_t b = 0; b < vb->B; b++) {
            const std::vector<double> row = array_row_doubles(pv, b);
            for (size_t r = 0; r < (size_t)sig.vec_size / pv.n; r++) std::copy(row.begin(), row.end(), a.mutable_data() + b * sig.vec_size + r * pv.n);
          }
          out[py::str(kv.first)] = py::array(a);
        }
        return out;
      }, py::arg("enc_outputs"), py::arg("signature"), py::arg("dtype") = py::module_::import("numpy").attr("float64"), py::arg("device") = false,
           "decrypt a SEALValuationBatch (or a list of SEALValuations) into {name: ndarray[B, vec_size]}: up to 64 instances of one name per "
           "device call, written straight into the array's rows; float64 rows are decrypt_batch's doubles bit for bit, float32 rows are those "
           "doubles rounded to nearest-even on the device, uint8 rows the nearest integer (ties to even) clamped to [0, 255], NaN -> 0. "
           "device=True: every decrypted name is a DeviceArray [B, vec_size] in the key pair's device state instead (no device -> host copy, "
           "one wait at the end of the call); unencrypted outputs stay numpy arrays")
      // test hook: an unwritten DeviceArray [B, n] from the pool of the key pair's device state — what the pool hands out next
      .def("_device_array", [](HipSecret &s, size_t B, size_t n, py::object dtype) {
        const py::dtype dt = py::dtype::from_args(dtype);
        if (!s.on_device()) throw std::runtime_error("decrypt_array needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
        return std::make_shared<DeviceArray>(s.dev, dt.itemsize() == 8 ? EVAH_F64 : dt.itemsize() == 4 ? EVAH_F32 : EVAH_U8, B, n);
      }, py::arg("B"), py::arg("n"), py::arg("dtype"))
      .def("refresh", [](HipSecret &s, py::object enc, const CKKSSignature &sig, py::object rename, py::object inputs, uint64_t seed) -> py::object {
        const auto rn = rename.is_none() ? std::map<std::string, std::string>{} : rename.cast<std::map<std::string, std::string>>();
        const Valuation in = inputs.is_none() ? Valuation{} : inputs.cast<Valuation>();
        if (py::isinstance<HipValuationBatch>(enc)) return py::cast(s.refresh_batch(enc.cast<const HipValuationBatch &>(), sig, rn, in, seed));
        return py::cast(s.refresh(enc.cast<const HipValuation &>(), sig, rn, in, seed));
      }, py::arg("enc"), py::arg("signature"), py::arg("rename") = py::none(), py::arg("inputs") = py::none(), py::arg("seed") = 0,
           "Refresh (DESIGN.md 1.12): decrypt, divide by a power of two and encrypt again under this key pair, without decoding. enc: a "
           "SEALValuation or a SEALValuationBatch (the same kind comes back); signature: that of the program that will consume the result — "
           "every encrypted input `name` of it is made from enc[(rename or {}).get(name, name)] at the input's level and scale 2^b. The "
           "integer message M becomes floor((M + 2^(t-1)) / 2^t) with 2^t the ratio of the scales (0 <= t <= 62; ties towards +infinity). "
           "inputs: the consumer's unencrypted inputs. Randomness as encrypt_batch(..., device_sampling=True); seed != 0 is the reproducible "
           "test hook and not secret-grade. Every result is seeded (c0 + the 32-byte seed of c1)")
      .def("make_rekey_key", [](HipSecret &s, const HipPublic &target, uint64_t seed) { return s.make_rekey_key(target, seed); },
           py::arg("target_public_ctx"), py::arg("seed") = 0,
           "The RekeyKey from this key pair to the one `target_public_ctx` belongs to (same poly_modulus_degree and primes), made from the "
           "target's public key (DESIGN.md 1.13). Whoever holds it together with the target's secret key learns this secret key: that is "
           "inherent to proxy re-encryption. seed != 0 is the reproducible test hook and not secret-grade")
      .def("relin_round1", [](HipSecret &s, uint64_t seed) {
        auto r = s.relin_round1(seed);
        return py::make_tuple(r.first, r.second);
      }, py::arg("seed") = 0,
           "Round 1 of the collective relinearization-key generation (DESIGN.md 1.15): returns (eph, share1). share1 is this party's public "
           "RelinShare; eph is its ephemeral secret for relin_round2. Needs keys made by generate_keys(..., common_seed=). seed != 0 is the "
           "reproducible test hook and not secret-grade")
      .def("relin_round2", [](HipSecret &s, std::shared_ptr<RelinEphemeral> eph, std::shared_ptr<RelinShare> agg1, uint64_t seed) {
        return s.relin_round2(eph, agg1, seed);
      }, py::arg("eph"), py::arg("agg1"), py::arg("seed") = 0,
           "Round 2 (DESIGN.md 1.15): this party's RelinShare from its own eph of relin_round1 — which serves once — and the "
           "combine_relin_shares aggregate of ALL parties' round-1 shares. seed != 0 is the reproducible test hook and not secret-grade")
      .def("transfer_stats", [](HipSecret &s) {
        auto st = s.transfer_stats();
        py::dict d;
        d["ct_uploads"] = st[0]; d["ct_downloads"] = st[1]; d["pt_uploads"] = st[2]; d["pt_downloads"] = st[3];
        d["h2d_bytes"] = st[4]; d["d2h_bytes"] = st[5];
        return d;
      }, "ciphertext / plaintext transfers across the host boundary of the key pair's device state")
      .def("decrypt_share", [](HipSecret &s, py::object enc, uint32_t smudge_bits, uint64_t seed) {
        if (py::isinstance<HipValuationBatch>(enc)) return s.decrypt_share_batch(enc.cast<const HipValuationBatch &>(), smudge_bits, seed);
        return s.decrypt_share(enc.cast<const HipValuation &>(), smudge_bits, seed);
      }, py::arg("enc"), py::arg("smudge_bits"), py::arg("seed") = 0,
           "This party's decryption share of every encrypted value of enc (a SEALValuation or a SEALValuationBatch) under a collective key "
           "(DESIGN.md 1.14): h = c1 * s_p + NTT(E) with E uniform on [-2^smudge_bits, 2^smudge_bits), drawn on the GPU from a 32-byte key per "
           "value. smudge_bits (1..62) is the caller's security parameter and has no default: it should exceed the ciphertext's noise bits by "
           "the statistical security wanted, since a CKKS decryption leaks its noise and the flood is what hides it; 2^(smudge_bits + 2) times "
           "the number of parties must stay below the modulus of the value's level. seed != 0 is the reproducible test hook, not secret-grade. "
           "Unencrypted and raw values are skipped. Returns DecryptionShares for SEALPublic.combine_shares")
      .def("decrypt", &HipSecret::decrypt, py::arg("enc_outputs"), py::arg("signature"))
      .def("decrypt_batch", &HipSecret::decrypt_batch, py::arg("enc_outputs"), py::arg("signature"),
           "decrypt() of every valuation of a list, bit for bit; on the device up to 64 outputs of one name are decrypted and decoded in one call")
      .def_readwrite("device", &HipSecret::device, "device of the secret half's state when it is not shared with a public context")
      // test hook: the 32-byte keys generate_keys(..., seed != 0, device_sampling=True) drew from its secret stream —
      // {"secret": rk_s, "public": ek_pk, 0: the relinearization key's error keys [digits][32], Galois element: that key's};
      // empty for every other pair
      .def("_key_randomness", [](const HipSecret &s) {
        py::dict d;
        const auto &r = s.key_randomness;
        if (r.rk_s.empty()) return d;
        d["secret"] = py::bytes(reinterpret_cast<const char *>(r.rk_s.data()), r.rk_s.size());
        d["public"] = py::bytes(reinterpret_cast<const char *>(r.ek_pk.data()), r.ek_pk.size());
        for (auto &kv : r.ekeys) {
          py::array_t<uint8_t> a({(py::ssize_t)(kv.second.size() / 32), (py::ssize_t)32});
          std::memcpy(a.mutable_data(), kv.second.data(), kv.second.size());
          d[py::int_(kv.first)] = a;
        }
        return d;
      })
      // test hook (as relin_key() on the public side): the secret key under every key prime, NTT form [k][N]
      .def("_secret_key_ntt", [](const HipSecret &s) { return to_numpy(s.sk.s_ntt, {(py::ssize_t)s.host->k, (py::ssize_t)s.host->N}); });
}
