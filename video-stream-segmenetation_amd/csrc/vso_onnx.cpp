// vso_onnx.cpp — the protobuf wire reader behind vso_create: ModelProto bytes
// -> Graph (vso_onnx.h), and the float16 / bfloat16 conversions of the
// constants.  It takes a user's file: every read is bounded by the enclosing
// message, and anything cut short or of the wrong wire type is an error.
#include "vso_onnx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vso_onnx {

namespace {

// ---- protobuf wire format ---------------------------------------------------
struct PB {
  const uint8_t* p;
  const uint8_t* e;
  bool bad = false;
  bool more() const { return !bad && p < e; }
  uint64_t varint() {
    uint64_t r = 0;
    for (int s = 0; s < 64; s += 7) {
      if (p >= e) { bad = true; return 0; }
      const uint8_t c = *p++;
      r |= (uint64_t)(c & 0x7F) << s;
      if (c < 0x80) return r;
    }
    bad = true;
    return 0;
  }
  bool key(uint32_t& f, uint32_t& wt) {
    const uint64_t k = varint();
    f = (uint32_t)(k >> 3);
    wt = (uint32_t)(k & 7);
    return !bad;
  }
  PB sub() {
    const uint64_t n = varint();
    if (bad || n > (uint64_t)(e - p)) { bad = true; return PB{e, e}; }
    PB s{p, p + n};
    p += n;
    return s;
  }
  uint32_t fixed32() {
    if (e - p < 4) { bad = true; return 0; }
    uint32_t v;
    std::memcpy(&v, p, 4);
    p += 4;
    return v;
  }
  uint64_t fixed64() {
    if (e - p < 8) { bad = true; return 0; }
    uint64_t v;
    std::memcpy(&v, p, 8);
    p += 8;
    return v;
  }
  std::string str() {
    PB s = sub();
    return std::string(reinterpret_cast<const char*>(s.p), s.e - s.p);
  }
  void skip(uint32_t wt) {
    if (wt == 0) varint();
    else if (wt == 1) fixed64();
    else if (wt == 2) sub();
    else if (wt == 5) fixed32();
    else bad = true;
  }
  // fn(the sub-message) for each field `want` of this message; the rest skipped
  template <class F>
  void each(uint32_t want, F fn) {
    uint32_t f, wt;
    while (more() && key(f, wt)) {
      if (f == want) fn(sub());
      else skip(wt);
    }
  }
};

void read_int64s(PB& pb, uint32_t wt, std::vector<int64_t>& out) {
  if (wt == 2) {
    PB s = pb.sub();
    while (s.more()) out.push_back((int64_t)s.varint());
    pb.bad |= s.bad;
  } else {
    out.push_back((int64_t)pb.varint());
  }
}

void read_floats(PB& pb, uint32_t wt, std::vector<float>& out) {
  if (wt == 2) {
    PB s = pb.sub();
    while (s.more()) {
      const uint32_t u = s.fixed32();
      float f;
      std::memcpy(&f, &u, 4);
      out.push_back(f);
    }
    pb.bad |= s.bad;
  } else {
    const uint32_t u = pb.fixed32();
    float f;
    std::memcpy(&f, &u, 4);
    out.push_back(f);
  }
}

// raw_data as whole elements of T (a trailing partial element is dropped)
template <class T>
std::vector<T> raw_as(const std::string& raw) {
  std::vector<T> v(raw.size() / sizeof(T));
  if (!v.empty()) std::memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}

bool parse_tensor(PB pb, std::string* name, Const* c, std::string* err) {
  int dt = DT_FLOAT;
  std::string raw;
  bool has_raw = false;
  std::vector<float> fl;
  std::vector<int64_t> i32, i64;
  std::vector<double> dbl;
  uint32_t f, wt;
  while (pb.more() && pb.key(f, wt)) {
    if (f == 1) read_int64s(pb, wt, c->dims);
    else if (f == 2) dt = (int)pb.varint();
    else if (f == 4) read_floats(pb, wt, fl);
    else if (f == 5) read_int64s(pb, wt, i32);
    else if (f == 7) read_int64s(pb, wt, i64);
    else if (f == 8) *name = pb.str();
    else if (f == 9) { raw = pb.str(); has_raw = true; }
    else if (f == 10) {
      if (wt == 2) {
        PB s = pb.sub();
        while (s.more()) { const uint64_t u = s.fixed64(); double d; std::memcpy(&d, &u, 8); dbl.push_back(d); }
      } else { const uint64_t u = pb.fixed64(); double d; std::memcpy(&d, &u, 8); dbl.push_back(d); }
    } else if (f == 14) {
      if (pb.varint() == 1) { *err = "external tensor data is not supported"; return false; }
    } else pb.skip(wt);
  }
  if (pb.bad) { *err = "malformed TensorProto"; return false; }
  c->dtype = dt;
  const int64_t n = c->numel();
  auto set_ints = [&](const std::vector<int64_t>& v) {
    c->is_int = true;
    c->i = v;
    c->f.assign(v.begin(), v.end());
  };
  switch (dt) {
    case DT_FLOAT:
      c->f = has_raw ? raw_as<float>(raw) : fl;
      break;
    case DT_FLOAT16: {
      std::vector<uint16_t> h;
      if (has_raw) h = raw_as<uint16_t>(raw);
      else for (int64_t v : i32) h.push_back((uint16_t)v);
      for (uint16_t v : h) c->f.push_back(half_to_float(v));
      c->f16 = true;
      break;
    }
    case DT_UINT4: case DT_INT4: {  // two per byte, low nibble first
      std::vector<int64_t> v;
      for (int64_t k = 0; k < n; ++k) {
        int q = 0;
        if (has_raw) {
          if ((size_t)(k / 2) >= raw.size()) break;
          q = ((uint8_t)raw[k / 2] >> ((k & 1) * 4)) & 15;
        } else {
          if ((size_t)(k / 2) >= i32.size()) break;
          q = ((int)i32[k / 2] >> ((k & 1) * 4)) & 15;
        }
        v.push_back(dt == DT_INT4 && q >= 8 ? q - 16 : q);
      }
      set_ints(v);
      break;
    }
    case DT_DOUBLE:
      if (has_raw) dbl = raw_as<double>(raw);
      c->f.assign(dbl.begin(), dbl.end());
      break;
    case DT_INT64:
      set_ints(has_raw ? raw_as<int64_t>(raw) : i64);
      break;
    case DT_INT32: case DT_INT8: case DT_UINT8: case DT_BOOL: {
      std::vector<int64_t> v;
      if (has_raw) {
        const size_t es = dt == DT_INT32 ? 4 : 1;
        for (size_t k = 0; k + es <= raw.size(); k += es) {
          if (dt == DT_INT32) { int32_t x; std::memcpy(&x, raw.data() + k, 4); v.push_back(x); }
          else if (dt == DT_INT8) v.push_back((int8_t)raw[k]);
          else v.push_back((uint8_t)raw[k]);
        }
      } else v = i32;
      set_ints(v);
      break;
    }
    case DT_UINT16: case DT_INT16: case DT_FLOAT8E4M3FN: case DT_FLOAT8E4M3FNUZ: case DT_FLOAT8E5M2:
    case DT_FLOAT8E5M2FNUZ:
      // a type no operator here computes on: the tensor keeps its type and dims, not its values, so that the
      // node reading it is refused by name (the planner: opaque_type) instead of the whole model by the reader
      // (only as many elements as the tensor's own data holds: a size that does not match its dims fails below)
      if ((int64_t)(has_raw ? raw.size() / (dt == DT_UINT16 || dt == DT_INT16 ? 2 : 1) : i32.size()) == n)
        c->f.assign((size_t)std::max<int64_t>(n, 0), 0.f);
      break;
    default:
      *err = "tensor data type " + std::to_string(dt) + " is not supported";
      return false;
  }
  if ((int64_t)c->f.size() != n) { *err = "tensor '" + *name + "' size does not match its dims"; return false; }
  return true;
}

bool parse_attr(PB pb, std::string* name, Attr* a, std::string* err) {
  uint32_t f, wt;
  while (pb.more() && pb.key(f, wt)) {
    if (f == 1) *name = pb.str();
    else if (f == 2) { const uint32_t u = pb.fixed32(); std::memcpy(&a->f, &u, 4); a->has_f = true; }
    else if (f == 3) { a->i = (int64_t)pb.varint(); a->has_i = true; }
    else if (f == 4) { a->s = pb.str(); a->has_s = true; }
    else if (f == 5) { std::string tn; if (!parse_tensor(pb.sub(), &tn, &a->t, err)) return false; a->has_t = true; }
    else if (f == 7) read_floats(pb, wt, a->fs);
    else if (f == 8) read_int64s(pb, wt, a->is);
    else pb.skip(wt);
  }
  if (pb.bad) { *err = "malformed AttributeProto"; return false; }
  return true;
}

// ValueInfoProto {name = 1, type = 2 {tensor_type = 1 {elem_type = 1, shape = 2 {dim = 1 {dim_value = 1}}}}}
bool parse_value_info(PB pb, IO* io) {
  uint32_t f, wt;
  while (pb.more() && pb.key(f, wt)) {
    if (f == 1) io->name = pb.str();
    else if (f == 2)
      pb.sub().each(1, [&](PB tt) {
        uint32_t f3, w3;
        while (tt.more() && tt.key(f3, w3)) {
          if (f3 == 1 && w3 == 0) io->elem_type = (int)tt.varint();
          else if (f3 == 2 && w3 == 2) tt.sub().each(1, [&](PB dm) {
            int64_t d = -1;
            uint32_t f5, w5;
            while (dm.more() && dm.key(f5, w5)) {
              if (f5 == 1) d = (int64_t)dm.varint();
              else dm.skip(w5);
            }
            io->dims.push_back(d);
          });
          else tt.skip(w3);
        }
      });
    else pb.skip(wt);
  }
  return !pb.bad;
}

bool parse_node(PB np, Node* nd, std::string* err) {
  uint32_t f, wt;
  while (np.more() && np.key(f, wt)) {
    if (f == 1) nd->in.push_back(np.str());
    else if (f == 2) nd->out.push_back(np.str());
    else if (f == 3) nd->name = np.str();
    else if (f == 4) nd->op = np.str();
    else if (f == 5) {
      std::string an;
      Attr a;
      if (!parse_attr(np.sub(), &an, &a, err)) return false;
      nd->attrs[an] = a;
    } else np.skip(wt);
  }
  if (np.bad) { *err = "malformed NodeProto"; return false; }
  return true;
}

}  // namespace

bool parse_model(const uint8_t* data, size_t n, Graph* g, std::string* err) {
  PB m{data, data + n};
  uint32_t f, wt;
  bool have_graph = false;
  while (m.more() && m.key(f, wt)) {
    if (f == 8) {  // opset_import: OperatorSetIdProto {domain = 1, version = 2}
      PB op = m.sub();
      std::string domain;
      int64_t version = 0;
      uint32_t f2, w2;
      while (op.more() && op.key(f2, w2)) {
        if (f2 == 1) domain = op.str();
        else if (f2 == 2) version = (int64_t)op.varint();
        else op.skip(w2);
      }
      if (op.bad) { *err = "malformed OperatorSetIdProto"; return false; }
      if (domain.empty() || domain == "ai.onnx") g->opset = std::max(g->opset, version);
      continue;
    }
    if (f != 7) { m.skip(wt); continue; }
    have_graph = true;
    PB gp = m.sub();
    uint32_t f2, w2;
    while (gp.more() && gp.key(f2, w2)) {
      if (f2 == 1) {
        Node nd;
        if (!parse_node(gp.sub(), &nd, err)) return false;
        g->nodes.push_back(nd);
      } else if (f2 == 5) {
        std::string tn;
        Const c;
        if (!parse_tensor(gp.sub(), &tn, &c, err)) return false;
        g->inits[tn] = c;
      } else if (f2 == 11 || f2 == 12) {
        IO io;
        if (!parse_value_info(gp.sub(), &io)) { *err = "malformed ValueInfoProto"; return false; }
        (f2 == 11 ? g->inputs : g->outputs).push_back(io);
      } else gp.skip(w2);
    }
    if (gp.bad) { *err = "malformed GraphProto"; return false; }
  }
  if (m.bad || !have_graph) { *err = "not an ONNX ModelProto (no graph)"; return false; }
  // graph inputs that are initializers are constants, not feeds
  std::vector<IO> feeds;
  for (const IO& io : g->inputs)
    if (!g->inits.count(io.name)) feeds.push_back(io);
  g->inputs = feeds;
  return true;
}

float half_to_float(uint16_t h) {
  const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31, m = h & 1023;
  uint32_t u;
  if (e == 0) {
    if (m == 0) u = s;
    else {  // subnormal
      float f = std::ldexp((float)m, -24);
      std::memcpy(&u, &f, 4);
      u |= s;
    }
  } else if (e == 31) {
    u = s | 0x7F800000u | (m << 13);
  } else {
    u = s | ((e + 112) << 23) | (m << 13);
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

float round_half(float f) {
  const float a = std::fabs(f);
  if (!(a < INFINITY)) return f;  // inf / nan
  float q;
  if (a >= 65520.f) q = INFINITY;
  else if (a < 6.103515625e-05f) q = std::nearbyint(a * 16777216.f) / 16777216.f;  // subnormal: quantum 2^-24
  else {
    int e = 0;
    (void)std::frexp(a, &e);  // a in [2^(e-1), 2^e): 11 significant bits
    const float sc = std::ldexp(1.f, 11 - e);
    q = std::nearbyint(a * sc) / sc;
  }
  return std::copysign(q, f);
}

}  // namespace vso_onnx
