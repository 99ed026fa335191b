// vso_onnx.h — an ONNX model as the sessions (include/vso.h) read it: the
// graph's nodes, attributes, initializers and inputs / outputs out of the
// protobuf bytes (vso_onnx.cpp), and the host evaluation of constant nodes and
// view shapes (vso_fold.cpp).  Plain C++17, no GPU: vso_onnx_check.cpp runs
// both units under the host sanitizers (make onnx-asan).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// (internal to libvss.so: nothing here joins its export table)
namespace vso_onnx __attribute__((visibility("hidden"))) {

// TensorProto.DataType
enum { DT_FLOAT = 1, DT_UINT8 = 2, DT_INT8 = 3, DT_UINT16 = 4, DT_INT16 = 5, DT_INT32 = 6, DT_INT64 = 7, DT_BOOL = 9, DT_FLOAT16 = 10,
       DT_DOUBLE = 11, DT_FLOAT8E4M3FN = 17, DT_FLOAT8E4M3FNUZ = 18, DT_FLOAT8E5M2 = 19, DT_FLOAT8E5M2FNUZ = 20,
       DT_UINT4 = 21, DT_INT4 = 22 };
// 16-bit integer and float8 tensors are read as their type and dims only (vso_onnx.cpp: parse_tensor)
inline bool opaque_type(int dt) { return dt == DT_UINT16 || dt == DT_INT16 || (dt >= DT_FLOAT8E4M3FN && dt <= DT_FLOAT8E5M2FNUZ); }

// A constant tensor (initializer / attribute / folded value).
struct Const {
  std::vector<int64_t> dims;
  bool is_int = false;
  bool f16 = false;        // float16-typed (values are exact halves)
  int dtype = 0;           // an initializer's / tensor attribute's TensorProto.DataType (0: a computed value)
  std::vector<float> f;    // float data (also filled for ints, as doubles would be)
  std::vector<int64_t> i;  // integer data
  int64_t numel() const {
    int64_t n = 1;
    for (int64_t d : dims) n *= d;
    return n;
  }
};

struct Attr {
  bool has_f = false, has_i = false, has_s = false, has_t = false;
  float f = 0.f;
  int64_t i = 0;
  std::string s;
  std::vector<float> fs;
  std::vector<int64_t> is;
  Const t;
};

struct Node {
  std::string op, name;
  std::vector<std::string> in, out;
  std::map<std::string, Attr> attrs;
  int64_t ai(const char* k, int64_t d) const {
    auto it = attrs.find(k);
    return it != attrs.end() && it->second.has_i ? it->second.i : d;
  }
  float af(const char* k, float d) const {
    auto it = attrs.find(k);
    return it != attrs.end() && it->second.has_f ? it->second.f : d;
  }
  std::string as(const char* k, const char* d) const {
    auto it = attrs.find(k);
    return it != attrs.end() && it->second.has_s ? it->second.s : std::string(d);
  }
  bool has(const char* k) const { return attrs.count(k) != 0; }
  std::vector<int64_t> ais(const char* k) const {
    auto it = attrs.find(k);
    return it != attrs.end() ? it->second.is : std::vector<int64_t>{};
  }
};

struct IO {
  std::string name;
  std::vector<int64_t> dims;  // -1 = symbolic
  int elem_type = 0;          // the declared TensorProto.DataType (0: none stated)
};

struct Graph {
  std::vector<Node> nodes;
  std::map<std::string, Const> inits;
  std::vector<IO> inputs, outputs;  // inputs: the feeds (graph inputs that are initializers left out)
  int64_t opset = 0;  // the default domain's opset_import version (0: none stated)
};

// ModelProto bytes -> Graph; false with *err set on anything malformed or unsupported
bool parse_model(const uint8_t* data, size_t n, Graph* g, std::string* err);

float half_to_float(uint16_t h);
// f -> bfloat16 / float16 bits, round to nearest even (NaN stays NaN; the
// GPU's __float2half_rn).  Inline: the planner converts every weight.
inline uint16_t float_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline uint16_t float_to_half_bits(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t b;
  std::memcpy(&b, &h, 2);
  return b;
}
// f -> the nearest float16 value (ties to even), as a float: what a Cast to
// FLOAT16 or a float16-typed result holds
float round_half(float f);

// A node input as the host evaluation sees it: its shape, and its value when
// it is a constant.  An absent optional input has neither.
struct Operand {
  const std::vector<int64_t>* shape = nullptr;
  const Const* c = nullptr;
  explicit operator bool() const { return shape != nullptr; }
};

// The value of a node whose inputs are all constants (Shape: of any input),
// as the exporters' shape arithmetic and weight reshapes need it.
bool fold(const Node& nd, const std::vector<Operand>& in, Const* out, std::string* err);
// Output shape of the view ops (Reshape, Flatten, Squeeze, Unsqueeze).
bool infer_view(const Node& nd, const std::vector<Operand>& in, std::vector<int64_t>* out, std::string* err);

}  // namespace vso_onnx
