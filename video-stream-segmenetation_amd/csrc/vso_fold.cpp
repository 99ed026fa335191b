// vso_fold.cpp — host evaluation at session create (vso_onnx.h): `fold`
// computes a node whose inputs are all constants (the exporters' Shape /
// Gather / Concat / ... arithmetic, weight reshapes, DequantizeLinear), and
// `infer_view` the output shape of Reshape / Flatten / Squeeze / Unsqueeze.
// Functions of the node and its operands alone; no GPU.
#include "vso_onnx.h"

#include <algorithm>
#include <cmath>

namespace vso_onnx {

namespace {

bool fail(std::string* err, const std::string& m) {
  *err = m;
  return false;
}

std::vector<int64_t> ints(const Const& c) { return c.is_int ? c.i : std::vector<int64_t>(c.f.begin(), c.f.end()); }

bool fold_constant(const Node& nd, Const& r, std::string* err) {
  auto it = nd.attrs.find("value");
  if (it != nd.attrs.end() && it->second.has_t) r = it->second.t;
  else if (nd.has("value_float")) { r.f = {nd.af("value_float", 0)}; }
  else if (nd.has("value_int")) { r.is_int = true; r.i = {nd.ai("value_int", 0)}; r.f = {(float)r.i[0]}; }
  else if (nd.has("value_ints")) { r.is_int = true; r.i = nd.ais("value_ints"); r.dims = {(int64_t)r.i.size()}; r.f.assign(r.i.begin(), r.i.end()); }
  else if (nd.has("value_floats")) { r.f = nd.attrs.at("value_floats").fs; r.dims = {(int64_t)r.f.size()}; }
  else return fail(err, "Constant without a supported value");
  return true;
}

void fold_shape(const Node& nd, const std::vector<int64_t>& shape, Const& r) {
  r.is_int = true;
  r.i = shape;
  int64_t st = nd.ai("start", 0), en = nd.ai("end", (int64_t)r.i.size());
  const int64_t rk = (int64_t)r.i.size();
  if (st < 0) st += rk;
  if (en < 0) en += rk;
  st = std::clamp<int64_t>(st, 0, rk);
  en = std::clamp<int64_t>(en, 0, rk);
  r.i = std::vector<int64_t>(r.i.begin() + st, r.i.begin() + std::max(st, en));
  r.dims = {(int64_t)r.i.size()};
  r.f.assign(r.i.begin(), r.i.end());
}

void fold_constant_of_shape(const Node& nd, const Const& shape, Const& r) {
  r.dims = ints(shape);
  float v = 0.f;
  bool is_int = false;
  auto it = nd.attrs.find("value");
  if (it != nd.attrs.end() && it->second.has_t && !it->second.t.f.empty()) {
    v = it->second.t.f[0];
    is_int = it->second.t.is_int;
  }
  r.is_int = is_int;
  r.f.assign((size_t)r.numel(), v);
  if (is_int) r.i.assign((size_t)r.numel(), (int64_t)v);
}

// Identity, Cast, Floor, Ceil
void fold_elementwise(const Node& nd, const Const& x, Const& r) {
  r = x;
  if (nd.op == "Cast") {
    const int64_t to = nd.ai("to", DT_FLOAT);
    const bool to_int = to == DT_INT64 || to == DT_INT32 || to == DT_INT8 || to == DT_UINT8 || to == DT_BOOL;
    if (to_int && !r.is_int) { r.i.clear(); for (float v : r.f) r.i.push_back((int64_t)v); }
    r.is_int = to_int;
    r.dtype = (int)to;
    r.f16 = to == DT_FLOAT16;
    if (r.f16)
      for (float& v : r.f) v = round_half(v);
  } else if (nd.op == "Floor" || nd.op == "Ceil") {
    for (float& v : r.f) v = nd.op == "Floor" ? std::floor(v) : std::ceil(v);
  } else if (nd.op == "Sqrt" || nd.op == "Erf") {  // (float constants: an attention scale sqrt(d), a GELU table)
    for (float& v : r.f) v = (float)(nd.op == "Sqrt" ? std::sqrt((double)v) : std::erf((double)v));
  }
}

// Pow of a float constant by one constant exponent
bool fold_pow(const Node& nd, const Const& x, const Const& e, Const& r, std::string* err) {
  if (x.is_int || e.numel() != 1 || e.f.empty()) return fail(err, "Pow '" + nd.name + "': a float constant to one constant exponent only");
  r = x;
  for (float& v : r.f) v = (float)std::pow((double)v, (double)e.f[0]);
  return true;
}

// Add, Sub, Mul, Div with broadcasting on small constant tensors
bool fold_arith(const Node& nd, const Const& a, const Const& b, Const& r, std::string* err) {
  const std::string& op = nd.op;
  const bool both_int = a.is_int && b.is_int;
  const size_t ra = a.dims.size(), rb = b.dims.size(), rk = std::max(ra, rb);
  r.dims.assign(rk, 1);
  for (size_t d = 0; d < rk; ++d) {
    const int64_t da = d + ra >= rk ? a.dims[d + ra - rk] : 1, db = d + rb >= rk ? b.dims[d + rb - rk] : 1;
    if (da != db && da != 1 && db != 1) return fail(err, nd.op + ": incompatible constant shapes");
    r.dims[d] = std::max(da, db);
  }
  const int64_t n = r.numel();
  r.is_int = both_int;
  for (int64_t k = 0; k < n; ++k) {
    int64_t ka = 0, kb = 0, rem = k, sa = 1, sb = 1;
    for (int d = (int)rk - 1; d >= 0; --d) {
      const int64_t id = rem % r.dims[d];
      rem /= r.dims[d];
      const int64_t da = d + (int)ra >= (int)rk ? a.dims[d + ra - rk] : 1;
      const int64_t db = d + (int)rb >= (int)rk ? b.dims[d + rb - rk] : 1;
      if (da > 1) ka += id * sa;
      if (db > 1) kb += id * sb;
      sa *= da;
      sb *= db;
    }
    if (both_int) {
      const int64_t x = a.i[ka], y = b.i[kb];
      int64_t v = op == "Add" ? x + y : op == "Sub" ? x - y : op == "Mul" ? x * y
                                                                   : (y ? (int64_t)std::floor((double)x / y) : 0);
      r.i.push_back(v);
      r.f.push_back((float)v);
    } else {
      const double x = a.f[ka], y = b.f[kb];
      r.f.push_back((float)(op == "Add" ? x + y : op == "Sub" ? x - y : op == "Mul" ? x * y : x / y));
    }
  }
  return true;
}

// y = (x - zero_point) * scale: per tensor, per axis, or blocked along the
// axis (opset 21 block_size); int8/uint8/int4/uint4 weights
bool fold_dequantize(const Node& nd, const Const& x, const Const& sc, const Const* zp, Const& r, std::string* err) {
  if (!x.is_int) return fail(err, "DequantizeLinear: integer input expected");
  const int64_t rk = (int64_t)x.dims.size();
  int64_t ax = nd.ai("axis", 1);
  if (ax < 0) ax += rk;
  const int64_t bs = nd.ai("block_size", 0);
  const int64_t n = x.numel(), ns = sc.numel();
  int64_t inner = 1;
  for (int64_t k = ax + 1; k < rk; ++k) inner *= x.dims[k];
  const int64_t da = rk > 0 && ax < rk ? x.dims[ax] : 1;
  const int64_t sda = bs > 0 && ax < (int64_t)sc.dims.size() ? sc.dims[ax] : 1;
  if (ns != 1 && (ax < 0 || ax >= rk)) return fail(err, "DequantizeLinear: bad axis");
  if (ns != 1 && bs == 0 && ns != da) return fail(err, "DequantizeLinear: per-axis scale size mismatch");
  if (bs > 0 && (sda != (da + bs - 1) / bs || ns != n / da * sda))
    return fail(err, "DequantizeLinear: blocked scale shape mismatch");
  if (zp && zp->numel() != ns) return fail(err, "DequantizeLinear: zero point shape differs from the scale's");
  r.dims = x.dims;
  r.f.resize((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    int64_t si = 0;
    if (ns != 1) {
      const int64_t ia = (k / inner) % da;
      if (bs == 0) si = ia;
      else si = ((k / (inner * da)) * sda + ia / bs) * inner + k % inner;
    }
    const double q = (double)x.i[k] - (zp ? (double)zp->i[si] : 0.0);
    float v = (float)(q * (double)sc.f[si]);
    if (sc.f16) v = round_half(v);
    r.f[k] = v;
  }
  r.f16 = sc.f16;
  return true;
}

void fold_gather(const Node& nd, const Const& d, const Const& ix, Const& r) {
  int64_t ax = nd.ai("axis", 0);
  const int64_t rk = (int64_t)d.dims.size();
  if (ax < 0) ax += rk;
  int64_t outer = 1, inner = 1;
  for (int64_t k = 0; k < ax; ++k) outer *= d.dims[k];
  for (int64_t k = ax + 1; k < rk; ++k) inner *= d.dims[k];
  const std::vector<int64_t> idx = ints(ix);
  for (int64_t k = 0; k < ax; ++k) r.dims.push_back(d.dims[k]);
  for (int64_t v : ix.dims) r.dims.push_back(v);
  for (int64_t k = ax + 1; k < rk; ++k) r.dims.push_back(d.dims[k]);
  r.is_int = d.is_int;
  for (int64_t o = 0; o < outer; ++o)
    for (int64_t j : idx) {
      const int64_t jj = j < 0 ? j + d.dims[ax] : j;
      for (int64_t q = 0; q < inner; ++q) {
        const int64_t src = (o * d.dims[ax] + jj) * inner + q;
        r.f.push_back(d.f[src]);
        if (d.is_int) r.i.push_back(d.i[src]);
      }
    }
}

void fold_concat(const Node& nd, const std::vector<Operand>& in, Const& r) {
  int64_t ax = nd.ai("axis", 0);
  const int64_t rk = (int64_t)in[0].c->dims.size();
  if (ax < 0) ax += rk;
  r.dims = in[0].c->dims;
  r.dims[ax] = 0;
  bool all_int = true;
  for (const Operand& v : in) { r.dims[ax] += v.c->dims[ax]; all_int = all_int && v.c->is_int; }
  int64_t outer = 1;
  for (int64_t k = 0; k < ax; ++k) outer *= r.dims[k];
  r.is_int = all_int;
  for (int64_t o = 0; o < outer; ++o)
    for (const Operand& v : in) {
      const int64_t blk = v.c->numel() / std::max<int64_t>(outer, 1);
      for (int64_t q = 0; q < blk; ++q) {
        r.f.push_back(v.c->f[o * blk + q]);
        if (all_int) r.i.push_back(v.c->i[o * blk + q]);
      }
    }
}

bool fold_slice(const std::vector<Operand>& in, Const& r, std::string* err) {
  const Const& d = *in[0].c;
  if (d.dims.size() != 1) return fail(err, "Slice of a constant: rank 1 only");
  const std::vector<int64_t> st = ints(*in[1].c), en = ints(*in[2].c);
  const std::vector<int64_t> stp = in.size() > 4 && in[4] ? ints(*in[4].c) : std::vector<int64_t>{1};
  const int64_t L = d.dims[0];
  int64_t a = st[0] < 0 ? st[0] + L : st[0], b = en[0] < 0 ? en[0] + L : en[0];
  const int64_t step = stp[0];
  a = std::clamp<int64_t>(a, 0, L);
  b = std::clamp<int64_t>(b, step > 0 ? 0 : -1, L);
  r.is_int = d.is_int;
  for (int64_t k = a; step > 0 ? k < b : k > b; k += step) {
    r.f.push_back(d.f[k]);
    if (d.is_int) r.i.push_back(d.i[k]);
  }
  r.dims = {(int64_t)r.f.size()};
  return true;
}

void fold_transpose(const Node& nd, const Const& d, Const& r) {
  std::vector<int64_t> perm = nd.ais("perm");
  const size_t rk = d.dims.size();
  if (perm.empty()) for (size_t k = 0; k < rk; ++k) perm.push_back((int64_t)(rk - 1 - k));
  r.dims.resize(rk);
  for (size_t k = 0; k < rk; ++k) r.dims[k] = d.dims[perm[k]];
  std::vector<int64_t> st(rk, 1);
  for (int k = (int)rk - 2; k >= 0; --k) st[k] = st[k + 1] * d.dims[k + 1];
  const int64_t n = r.numel();
  r.is_int = d.is_int;
  for (int64_t o = 0; o < n; ++o) {
    int64_t rem = o, src = 0;
    for (int k = (int)rk - 1; k >= 0; --k) {
      src += (rem % r.dims[k]) * st[perm[k]];
      rem /= r.dims[k];
    }
    r.f.push_back(d.f[src]);
    if (d.is_int) r.i.push_back(d.i[src]);
  }
}

}  // namespace

bool fold(const Node& nd, const std::vector<Operand>& in, Const* out, std::string* err) {
  const std::string& op = nd.op;
  Const r;
  if (op == "Constant") {
    if (!fold_constant(nd, r, err)) return false;
  } else if (op == "Shape") fold_shape(nd, *in[0].shape, r);
  else if (op == "ConstantOfShape") fold_constant_of_shape(nd, *in[0].c, r);
  else if (op == "Identity" || op == "Cast" || op == "Floor" || op == "Ceil") fold_elementwise(nd, *in[0].c, r);
  else if ((op == "Sqrt" || op == "Erf") && !in[0].c->is_int) fold_elementwise(nd, *in[0].c, r);
  else if (op == "Pow" && in.size() == 2) {
    if (!fold_pow(nd, *in[0].c, *in[1].c, r, err)) return false;
  }
  else if (op == "Add" || op == "Sub" || op == "Mul" || op == "Div") {
    if (!fold_arith(nd, *in[0].c, *in[1].c, r, err)) return false;
  } else if (op == "DequantizeLinear") {
    if (!fold_dequantize(nd, *in[0].c, *in[1].c, in.size() > 2 && in[2] ? in[2].c : nullptr, r, err)) return false;
  } else if (op == "Gather") fold_gather(nd, *in[0].c, *in[1].c, r);
  else if (op == "Unsqueeze" || op == "Squeeze" || op == "Reshape" || op == "Flatten") {
    r = *in[0].c;
    if (!infer_view(nd, in, &r.dims, err)) return false;
  } else if (op == "Concat") fold_concat(nd, in, r);
  else if (op == "Slice") {
    if (!fold_slice(in, r, err)) return false;
  } else if (op == "Transpose") fold_transpose(nd, *in[0].c, r);
  else return fail(err, "cannot evaluate constant " + op + " (node '" + nd.name + "')");
  if (r.f.size() != (size_t)r.numel()) return fail(err, "constant " + op + " produced a malformed tensor");
  *out = r;
  return true;
}

bool infer_view(const Node& nd, const std::vector<Operand>& in, std::vector<int64_t>* out, std::string* err) {
  const std::vector<int64_t> x = *in[0].shape;  // (a copy: `out` may be the operand's own dims)
  const int64_t rk = (int64_t)x.size();
  const Const* c1 = in.size() > 1 ? in[1].c : nullptr;
  auto axes_of = [&](int64_t out_rank) -> std::vector<int64_t> {
    std::vector<int64_t> a = nd.ais("axes");
    if (a.empty() && c1) a = ints(*c1);
    for (int64_t& v : a) if (v < 0) v += out_rank;
    std::sort(a.begin(), a.end());
    return a;
  };
  if (nd.op == "Reshape") {
    if (!c1) return fail(err, "Reshape needs a constant shape");
    std::vector<int64_t> shp = ints(*c1);
    const bool allowzero = nd.ai("allowzero", 0) != 0;
    int64_t known = 1, neg = -1;
    for (size_t k = 0; k < shp.size(); ++k) {
      if (shp[k] == 0 && !allowzero) shp[k] = k < x.size() ? x[k] : 1;
      if (shp[k] == -1) neg = (int64_t)k;
      else known *= shp[k];
    }
    int64_t total = 1;
    for (int64_t d : x) total *= d;
    if (neg >= 0) shp[neg] = known ? total / known : 0;
    *out = shp;
  } else if (nd.op == "Flatten") {
    int64_t ax = nd.ai("axis", 1);
    if (ax < 0) ax += rk;
    int64_t a = 1, b = 1;
    for (int64_t k = 0; k < rk; ++k) (k < ax ? a : b) *= x[k];
    *out = {a, b};
  } else if (nd.op == "Squeeze") {
    std::vector<int64_t> axes = axes_of(rk);
    out->clear();
    for (int64_t k = 0; k < rk; ++k) {
      const bool drop = axes.empty() ? x[k] == 1 : std::binary_search(axes.begin(), axes.end(), k);
      if (!drop) out->push_back(x[k]);
    }
  } else {  // Unsqueeze
    std::vector<int64_t> a0 = nd.ais("axes");
    if (a0.empty() && c1 && c1->is_int) a0 = c1->i;
    const int64_t orank = rk + (int64_t)a0.size();
    std::vector<int64_t> axes = axes_of(orank);
    out->clear();
    size_t j = 0;
    for (int64_t k = 0; k < orank; ++k) {
      if (std::binary_search(axes.begin(), axes.end(), k)) out->push_back(1);
      else out->push_back(x[j++]);
    }
  }
  int64_t a = 1, b = 1;
  for (int64_t d : x) a *= d;
  for (int64_t d : *out) b *= d;
  if (a != b) return fail(err, nd.op + " '" + nd.name + "': element count changes");
  return true;
}

}  // namespace vso_onnx
