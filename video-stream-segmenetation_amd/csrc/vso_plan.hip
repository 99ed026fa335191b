// vso_plan.hip — the ONNX sessions' planner: a parsed Graph (vso_onnx.h) and
// the input shapes -> the session's launch list over preallocated HBM tensors
// (vso_session.h), at create.  Host code; the kernels are vso_kernels.hip,
// vso_conv.hip, vso_ir.hip, vso_deconv.hip, vso_attn.hip, vso_head.hip, vso_quant.hip and vso_dynq.hip.
//
// Planning rules:
//  * every shape is static once input 0's shape is fixed; nodes whose inputs
//    are all constants (the exporters' Shape/Gather/Concat/... arithmetic,
//    weight reshapes) are evaluated on the host (vso_fold.cpp);
//  * Reshape / Flatten / Squeeze / Unsqueeze / Identity alias their input;
//  * Conv absorbs a following BatchNormalization (weights folded), residual
//    Add and activation (Relu, Clip, PRelu, LeakyRelu, Sigmoid, Tanh,
//    HardSigmoid, HardSwish, and Mul(x, HardSigmoid(x)) as one) into one
//    launch when each intermediate has exactly one consumer; a ConvTranspose
//    absorbs them the same way (plan_conv_transpose);
//  * the fusions found before planning (find_*): IBNorm, strided residuals,
//    Concat inputs written in place, 2x upsamples computed by their consumer,
//    the erf form of GELU (one activation), attention (one k_attn launch),
//    the linear Resize in front of a class head (find_heads);
//  * Softmax / LogSoftmax / ArgMax / ReduceMax over the channel axis of a
//    rank-4 tensor are one k_class_head launch, which also takes that Resize,
//    a Softmax's channel selection and ArgMax -> Equal -> Cast (plan_*_head);
//  * a decomposed LayerNorm is found from its first ReduceMean when the walk
//    reaches it (find_layernorm); a MatMul by a constant absorbs a constant
//    bias Add, then an activation;
//  * QuantizeLinear / DequantizeLinear of runtime tensors are k_quantize /
//    k_dequantize over 8-bit buffers; DequantizeLinear -> Conv | Add [-> Relu |
//    Clip] -> QuantizeLinear run on the integers in one launch (find_qdq);
//  * DynamicQuantizeLinear is k_dyn_minmax + k_dyn_quantize, its scale and
//    zero point staying in HBM; ConvInteger / MatMulInteger are k_iconv_tile /
//    k_iconv_direct, and with the Cast -> Mul [-> Add] [-> Relu | Clip] behind
//    them one launch ending in float32 (find_dynq);
//  * every other runtime node is one launch, by the plan_<op> of its operator.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <set>

#include "vso_kernels.h"
#include "vso_session.h"

using namespace vso;
using namespace vso_onnx;

namespace {

struct Planner {
  using Ins = std::vector<Value*>;  // a node's inputs (null: an absent optional one)

  vso_session* s;
  Graph& g;
  std::map<std::string, Value> vals;
  std::map<std::string, int> consumers;
  std::set<size_t> done;  // node indices absorbed by a fused launch
  std::map<const void*, float*> dev_consts;
  std::string err;

  // ---- fusions found before planning (find_*; run) -------------------------
  // Add operands computed inside the consuming convolution's epilogue instead
  // of by their own launches: MaxPool(2x2, s2) -> [Pad of the channel axis] -> Add
  struct ResFuse {
    std::string src;          // the MaxPool's input, or the Pad's input
    int mode;                 // Epilogue::res_mode
    int pool_node, pad_node;  // the nodes left without a launch (-1: none)
  };
  std::map<std::string, ResFuse> res_fuse;  // by the Add operand's name (find_residual_fusions)
  // MODNet's IBNorm (Conv2dIBNormRelu; the authors' src/models/modnet.py):
  //   c = Conv(x); Concat(BN(Slice(c, 0:nb)), InstanceNorm(Slice(c, nb:M)), axis 1) [-> Relu]
  // with every intermediate used once.  The conv writes the concatenation
  // directly: the BatchNorm folded into its first nb output channels' weights,
  // the Relu applied to those channels in its epilogue; the InstanceNorm then
  // normalises channels nb .. M-1 in place (+ Relu).  Seven launches -> three.
  struct IbnFuse {
    int nb;
    size_t bn, inorm, concat;
    int relu;  // node index or -1
    std::string out;
  };
  std::map<size_t, IbnFuse> ibn;  // conv node -> its IBNorm (find_ibnorm)
  // Concat (axis 1) inputs whose producer — a convolution or a Resize — may
  // write them straight into the concatenation (find_concat_direct).
  // MODNet: 10 of its 13 Concat copies (the k_copy_rows launches).
  std::set<std::string> cat_direct;
  // 2x linear Resizes that may be computed inside their consumer convolution
  // (k_conv_tile_up), by graph structure (find_up_fusions)
  std::set<std::string> up_cand;

  // The hard-swish of exports before opset 14, Mul(x, HardSigmoid(x)) with the
  // HardSigmoid used by that Mul only: HardSigmoid node -> Mul node
  // (find_hswish).  The pair is one activation, x * clamp(alpha x + beta, 0, 1):
  // in the epilogue of x's producer when the two are all that reads x
  // (hswish_pair), else one k_unary launch (plan_activation).
  std::map<size_t, size_t> hswish;

  // Linear Resizes whose only reader is a Softmax, LogSoftmax, ArgMax or
  // ReduceMax (find_heads): candidates for the upsampled form of k_class_head
  std::set<std::string> head_up;
  // Index tensors: ArgMax outputs (and views of them) — float32 in HBM holding
  // exact integers, so a Cast of one to an integer type is an alias
  std::set<std::string> index_vals;

  // ---- work left by one node to a later one, by value name -----------------
  // Each entry is set by the producer's plan and cleared by the consumer that
  // takes it, or by the flush_* that launches it after all; run() fails if one
  // is left over.
  // pending_dw: a depthwise conv's output computed in its 1x1 consumer (input,
  //   producer).  Set: plan_conv (defer_depthwise).  Cleared: plan_conv of
  //   that consumer (feeds_pointwise guarantees it takes it).
  std::map<std::string, std::pair<const float*, DwPre>> pending_dw;
  // norm_pending: an InstanceNorm's apply step left to a k_conv_thin consumer.
  //   Set: plan_norm (defer).  Cleared: plan_conv's thin branch, or flush_norm.
  std::map<std::string, std::shared_ptr<NormParams>> norm_pending;
  // up_pending: a planned 2x Resize not yet launched.  Set: plan_resize.
  //   Cleared: plan_conv_dense (computed while staging), or flush_up.
  std::map<std::string, std::shared_ptr<ResizeParams>> up_pending;
  // cat_up: per Concat output, the channel ranges of its inputs still in
  //   up_pending.  Set: plan_concat.  Read by plan_conv_dense and flush_input
  //   (stale ranges are harmless: flush_up of a launched Resize does nothing).
  // head_pending: a Resize in head_up, planned without an output tensor.  Set:
  //   plan_resize.  Cleared: emit_head (the head interpolates on the fly), or
  //   flush_head, which allocates the tensor and launches k_resize after all.
  std::map<std::string, ResizeParams> head_pending;
  struct UpRange { std::string name; int c0, c1; };
  std::map<std::string, std::vector<UpRange>> cat_up;
  // cat_patch: per cat_direct value, patches re-pointing its producing
  //   launches' output into the concatenation (base: the input's first channel
  //   of image 0; ctot: the concatenation's channels).  Set: retarget_on_concat
  //   and plan_norm.  Applied by plan_concat, which then copies only the other
  //   inputs.
  std::map<std::string, std::vector<std::function<void(float*, int)>>> cat_patch;
  // cat_tail: a Concat's last input (whole 32-channel chunks on) left in its
  //   own tensor instead of copied in: its sole consumer, a convolution on
  //   k_conv_tile, reads those chunks from there (ConvTileParams::x2).  Set:
  //   plan_concat.  Cleared: plan_conv_dense, or flush_tail, which runs the
  //   copy.  MODNet: 3 copies of 8 x 3 / 32 x H x W planes (52 us of
  //   k_copy_rows at batch 8).
  struct CatTail {
    const float* x;
    int c0, C;
    std::function<bool()> copy;
  };
  std::map<std::string, CatTail> cat_tail;

  // launch a pending InstanceNorm apply step / fused Resize (by output name)
  // after all: its consumer cannot take it
  void flush_norm(const std::string& name) {
    auto nt = norm_pending.find(name);
    if (nt == norm_pending.end()) return;
    add("vso::k_norm_apply(vso::NormParams)", nt->second, launch_norm_apply);
    norm_pending.erase(nt);
  }
  void flush_up(const std::string& name) {
    flush_norm(name);
    auto it = up_pending.find(name);
    if (it == up_pending.end()) return;
    add(resize_kernel_name(*it->second), it->second, launch_resize);
    up_pending.erase(it);
  }
  bool flush_head(const std::string& name) {
    auto it = head_pending.find(name);
    if (it == head_pending.end()) return true;
    ResizeParams p = it->second;
    head_pending.erase(it);
    Value& v = vals[name];
    if ((v.buf = new_buf(v.numel())) < 0) return false;
    p.y = dptr(v);
    emit(resize_kernel_name(p), p, launch_resize);
    return true;
  }
  bool flush_tail(const std::string& name) {
    auto t = cat_tail.find(name);
    if (t == cat_tail.end()) return true;
    std::function<bool()> copy = std::move(t->second.copy);
    cat_tail.erase(t);
    return copy();
  }
  // a consumer that computes no upsample itself: its input's pending Resize and,
  // when the input is an in-place Concat, every pending upsampled input of it
  void flush_input(const std::string& name) {
    flush_tail(name);
    flush_up(name);
    auto cu = cat_up.find(name);
    if (cu != cat_up.end())
      for (const UpRange& u : cu->second) flush_up(u.name);
  }

  // ---- fusion discovery: what fills the sets and maps above ----------------
  bool slice_range(const Node& nd, int64_t C, int64_t* b, int64_t* e) {
    if (nd.op != "Slice" || nd.in.size() < 3) return false;
    auto cint = [&](size_t k, std::vector<int64_t>* out) {
      if (k >= nd.in.size() || nd.in[k].empty()) return false;
      Value* v = val(nd.in[k]);
      if (!v || !v->is_const || !v->c.is_int) return false;
      *out = v->c.i;
      return true;
    };
    std::vector<int64_t> st, en, ax{0}, sp{1};
    if (!cint(1, &st) || !cint(2, &en) || st.size() != 1 || en.size() != 1) return false;
    if (nd.in.size() > 3 && !nd.in[3].empty() && !cint(3, &ax)) return false;
    if (nd.in.size() > 4 && !nd.in[4].empty() && !cint(4, &sp)) return false;
    if (ax.size() != 1 || ax[0] != 1 || sp.size() != 1 || sp[0] != 1) return false;
    *b = std::clamp<int64_t>(st[0] < 0 ? st[0] + C : st[0], 0, C);
    *e = std::clamp<int64_t>(en[0] < 0 ? en[0] + C : en[0], 0, C);
    return true;
  }

  void find_ibnorm() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& cat = g.nodes[k];
      if (cat.op != "Concat" || cat.in.size() != 2 || cat.ai("axis", 0) != 1) continue;
      const int pbn = producer(cat.in[0]), pin = producer(cat.in[1]);
      if (pbn < 0 || pin < 0 || g.nodes[pbn].op != "BatchNormalization" || g.nodes[pin].op != "InstanceNormalization")
        continue;
      if (sole_consumer(cat.in[0], (size_t)pbn) != (int)k || sole_consumer(cat.in[1], (size_t)pin) != (int)k) continue;
      const Node &bn = g.nodes[pbn], &inn = g.nodes[pin];
      bool consts = bn.in.size() == 5 && inn.in.size() == 3;
      for (size_t q = 1; consts && q < bn.in.size(); ++q) consts = val(bn.in[q]) && val(bn.in[q])->is_const;
      for (size_t q = 1; consts && q < inn.in.size(); ++q) consts = val(inn.in[q]) && val(inn.in[q])->is_const;
      if (!consts) continue;
      const int sa = producer(bn.in[0]), sb = producer(inn.in[0]);
      if (sa < 0 || sb < 0 || sole_consumer(bn.in[0], (size_t)sa) != pbn || sole_consumer(inn.in[0], (size_t)sb) != pin)
        continue;
      const Node &la = g.nodes[sa], &lb = g.nodes[sb];
      if (la.op != "Slice" || lb.op != "Slice" || la.in[0] != lb.in[0]) continue;
      const std::string& c = la.in[0];
      const int pc = producer(c);
      if (pc < 0 || g.nodes[pc].op != "Conv" || consumers[c] != 2) continue;
      bool is_out = false;
      for (const IO& o : g.outputs) is_out = is_out || o.name == c;
      Value* wv = val(g.nodes[pc].in[1]);
      if (is_out || !wv || !wv->is_const || wv->c.dims.size() != 4) continue;
      const int64_t M = wv->c.dims[0];
      int64_t b0, e0, b1, e1;
      if (!slice_range(la, M, &b0, &e0) || !slice_range(lb, M, &b1, &e1)) continue;
      if (b0 != 0 || e0 != b1 || e1 != M || e0 <= 0 || e0 >= M) continue;
      if (val(bn.in[1])->c.numel() != e0 || val(inn.in[1])->c.numel() != M - e0) continue;
      IbnFuse f{(int)e0, (size_t)pbn, (size_t)pin, k, -1, cat.out[0]};
      const int r = sole_consumer(cat.out[0], k);
      if (r >= 0 && g.nodes[r].op == "Relu") {
        f.relu = r;
        f.out = g.nodes[r].out[0];
      }
      for (size_t q : {(size_t)sa, (size_t)sb, (size_t)pbn, (size_t)pin, k}) done.insert(q);
      if (f.relu >= 0) done.insert((size_t)f.relu);
      ibn[(size_t)pc] = f;
    }
  }

  bool channel_pad_only(const Node& nd) {
    if (nd.as("mode", "constant") != "constant" || nd.in.size() < 2) return false;
    Value* pv = val(nd.in[1]);
    if (!pv || !pv->is_const || !pv->c.is_int || pv->c.i.size() != 8) return false;
    if (nd.in.size() > 2 && !nd.in[2].empty()) {
      Value* cv = val(nd.in[2]);
      if (!cv || !cv->is_const || (!cv->c.f.empty() && cv->c.f[0] != 0.f)) return false;
    }
    if (nd.in.size() > 3 && !nd.in[3].empty()) return false;  // axes
    const std::vector<int64_t>& q = pv->c.i;
    for (int d = 0; d < 8; ++d)
      if (d != 5 && q[d] != 0) return false;
    return q[5] >= 0;
  }

  static bool pool_2x2(const Node& nd) {
    const std::vector<int64_t> k = nd.ais("kernel_shape"), st = nd.ais("strides"), pd = nd.ais("pads"),
                               dl = nd.ais("dilations");
    if (k != std::vector<int64_t>{2, 2} || st != std::vector<int64_t>{2, 2}) return false;
    for (int64_t v : pd) if (v != 0) return false;
    for (int64_t v : dl) if (v != 1) return false;
    return nd.ai("ceil_mode", 0) == 0 && nd.as("auto_pad", "NOTSET") == "NOTSET";
  }

  // MaxPool(2x2, stride 2, unpadded, floor) -> [Pad: zeros appended on the
  // channel axis only] -> Add(x, Conv(...)) where the Conv's output feeds only
  // that Add (so plan_conv absorbs the Add): the Pad / MaxPool launches are
  // dropped and the conv's epilogue reads the pool input (BlazeFace's and the
  // landmark net's strided residual path: 5 + 8 launches).
  void find_residual_fusions() {
    for (size_t a = 0; a < g.nodes.size(); ++a) {
      const Node& ad = g.nodes[a];
      if (ad.op != "Add" || ad.in.size() != 2 || ad.in[0] == ad.in[1]) continue;
      for (int side = 0; side < 2; ++side) {
        const std::string& cv = ad.in[side];
        const std::string& o = ad.in[1 - side];
        const int pc = producer(cv);
        if (pc < 0 || g.nodes[pc].op != "Conv" || sole_consumer(cv, (size_t)pc) != (int)a) continue;
        int pn = producer(o);
        if (pn < 0 || sole_consumer(o, (size_t)pn) != (int)a) continue;
        int mode = 0, pad_node = -1;
        std::string cur = o;
        if (g.nodes[pn].op == "Pad" && channel_pad_only(g.nodes[pn])) {
          pad_node = pn;
          cur = g.nodes[pn].in[0];
          mode = 1;
          pn = producer(cur);
          if (pn >= 0 && sole_consumer(cur, (size_t)pn) != pad_node) pn = -1;
        }
        int pool_node = -1;
        if (pn >= 0 && g.nodes[pn].op == "MaxPool" && pool_2x2(g.nodes[pn])) {
          pool_node = pn;
          cur = g.nodes[pn].in[0];
          mode = 2;
        }
        if (mode == 0) continue;
        // the source must exist when the Conv is planned: a graph input, or a value produced ahead of it
        if (producer(cur) > pc) continue;
        if (pad_node >= 0) done.insert((size_t)pad_node);
        if (pool_node >= 0) done.insert((size_t)pool_node);
        res_fuse[o] = ResFuse{cur, mode, pool_node, pad_node};
        break;
      }
    }
  }

  // Inputs of the Concats that may be written in place: used by that Concat
  // only, once, and neither a graph input / output nor a constant (whether the
  // producer can, and the Concat is on axis 1 of 4-D tensors, is decided when
  // they are planned: see cat_patch)
  void find_concat_direct() {
    std::set<std::string> fixed;
    for (const IO& o : g.inputs) fixed.insert(o.name);
    for (const IO& o : g.outputs) fixed.insert(o.name);
    for (auto& kv : g.inits) fixed.insert(kv.first);
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& cat = g.nodes[k];
      if (cat.op != "Concat" || done.count(k)) continue;
      for (const std::string& i : cat.in)
        if (!i.empty() && !fixed.count(i) && consumers[i] == 1) cat_direct.insert(i);
    }
  }

  // Resizes whose output feeds one convolution's input, directly or as an
  // input of a Concat (written in place) that feeds one: planned as pending
  // (plan_resize checks the kind: 2x linear half-pixel)
  void find_up_fusions() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& rs = g.nodes[k];
      if (rs.op != "Resize" || done.count(k)) continue;
      const std::string& o = rs.out[0];
      const int c = sole_consumer(o, k);
      if (c < 0) continue;
      const Node& cn = g.nodes[c];
      if (cn.op == "Conv" && cn.in[0] == o) {
        up_cand.insert(o);
      } else if (cn.op == "Concat" && cat_direct.count(o) && cn.ai("axis", 0) == 1) {
        const int cc = sole_consumer(cn.out[0], (size_t)c);
        if (cc >= 0 && g.nodes[cc].op == "Conv" && g.nodes[cc].in[0] == cn.out[0]) up_cand.insert(o);
      }
    }
  }

  void find_hswish() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& hs = g.nodes[k];
      if (hs.op != "HardSigmoid" || hs.in.size() != 1 || hs.out.empty() || g.inits.count(hs.in[0])) continue;
      const int m = sole_consumer(hs.out[0], k);
      if (m < 0 || g.nodes[m].op != "Mul" || g.nodes[m].in.size() != 2) continue;
      const Node& mul = g.nodes[m];
      const std::string& other = mul.in[0] == hs.out[0] ? mul.in[1] : mul.in[0];
      if (other == hs.in[0]) hswish[k] = (size_t)m;
    }
  }

  // `out` (a launch's output so far, written by node `last`) is read by a
  // decomposed hard-swish and by nothing else: the activation into *ep, the
  // HardSigmoid marked done; returns the Mul for the caller to absorb, or -1
  int hswish_pair(const std::string& out, size_t last, Epilogue* ep) {
    if (hswish.empty() || consumers[out] != 2) return -1;
    for (const IO& o : g.outputs)
      if (o.name == out) return -1;
    for (auto& kv : hswish) {
      const Node& hs = g.nodes[kv.first];
      if (kv.first <= last || hs.in[0] != out || done.count(kv.first) || done.count(kv.second)) continue;
      if (!act_of(hs, ep, 0)) return -1;
      ep->act = ACT_HSWISH;
      done.insert(kv.first);
      return (int)kv.second;
    }
    return -1;
  }

  // a constant operand as the find_* passes can know it before the walk: an
  // initializer, a value already folded, or a Constant node's tensor (into *tmp)
  const Const* const_of(const std::string& n, Const* tmp) {
    if (Value* v = val(n)) return v->is_const ? &v->c : nullptr;
    const int p = producer(n);
    std::string e;
    if (p < 0 || g.nodes[p].op != "Constant" || !fold(g.nodes[p], {}, tmp, &e)) return nullptr;
    return tmp;
  }
  bool scalar_of(const std::string& n, double* out) {
    Const t;
    const Const* c = const_of(n, &t);
    if (!c || c->numel() != 1 || c->f.empty()) return false;
    *out = c->f[0];
    return true;
  }
  static bool near(double v, double want) { return std::fabs(v - want) <= 1e-6 * std::fabs(want); }
  // nd = Mul / Add of `name` and a constant scalar (either order; a Div: name / scalar): the scalar
  bool with_scalar(const Node& nd, const std::string& name, double* c) {
    if (nd.in.size() != 2) return false;
    if (nd.in[0] == name && scalar_of(nd.in[1], c)) return true;
    return nd.op != "Div" && nd.in[1] == name && scalar_of(nd.in[0], c);
  }

  // The erf form of GELU (exports before opset 20):
  //   x * 0.5 * (1 + Erf(x / sqrt 2))
  // with the three-way product in either association — (x * (1 + erf)) * 0.5,
  // x * ((1 + erf) * 0.5), (x * 0.5) * (1 + erf) — x / sqrt 2 a Div or a Mul by
  // 1 / sqrt 2, the constants matched to 1e-6 relative, every interior value
  // used inside the pattern only.  The earliest of the five nodes (the head)
  // stands for the pattern, the others are done from here on: ACT_GELU in the
  // epilogue of x's producer when the pattern is all that reads x (gelu_pair),
  // else one k_unary launch when the walk reaches the head (plan_arith).
  struct GeluFuse {
    std::string x;
    size_t last;  // the node whose output is the pattern's
    std::vector<size_t> nodes;
  };
  std::map<size_t, GeluFuse> gelu;  // by head node (find_gelu)

  void find_gelu() {
    const double rt2 = std::sqrt(2.0);
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& ef = g.nodes[k];
      if (ef.op != "Erf" || ef.in.size() != 1 || done.count(k)) continue;
      const int pe = producer(ef.in[0]);
      if (pe < 0 || sole_consumer(ef.in[0], (size_t)pe) != (int)k) continue;
      const Node& sc = g.nodes[pe];
      if ((sc.op != "Div" && sc.op != "Mul") || sc.in.size() != 2) continue;
      double c;
      std::string x;
      for (int side = 0; side < 2 && x.empty(); ++side)
        if (with_scalar(sc, sc.in[side], &c) && near(c, sc.op == "Div" ? rt2 : 1.0 / rt2)) x = sc.in[side];
      Const tmp;
      if (x.empty() || const_of(x, &tmp)) continue;
      const int a = sole_consumer(ef.out[0], k);
      if (a < 0 || g.nodes[a].op != "Add" || !with_scalar(g.nodes[a], ef.out[0], &c) || !near(c, 1.0)) continue;
      const std::string& one_erf = g.nodes[a].out[0];
      const int m1 = sole_consumer(one_erf, (size_t)a);
      if (m1 < 0 || g.nodes[m1].op != "Mul" || g.nodes[m1].in.size() != 2) continue;
      const Node& mul1 = g.nodes[m1];
      const std::string& o1 = mul1.in[0] == one_erf ? mul1.in[1] : mul1.in[0];
      GeluFuse f{x, 0, {(size_t)pe, k, (size_t)a, (size_t)m1}};
      const int ph = producer(o1);
      if (o1 == x || (scalar_of(o1, &c) && near(c, 0.5))) {  // then the other of x and 0.5
        const int m2 = sole_consumer(mul1.out[0], (size_t)m1);
        if (m2 < 0 || g.nodes[m2].op != "Mul") continue;
        const bool ok = o1 == x ? with_scalar(g.nodes[m2], mul1.out[0], &c) && near(c, 0.5)
                                : g.nodes[m2].in.size() == 2 && (g.nodes[m2].in[0] == x) != (g.nodes[m2].in[1] == x);
        if (!ok) continue;
        f.last = (size_t)m2;
        f.nodes.push_back((size_t)m2);
      } else if (ph >= 0 && g.nodes[ph].op == "Mul" && sole_consumer(o1, (size_t)ph) == m1 &&
                 with_scalar(g.nodes[ph], x, &c) && near(c, 0.5)) {
        f.last = (size_t)m1;
        f.nodes.push_back((size_t)ph);
      } else {
        continue;
      }
      bool taken = false;
      for (size_t q : f.nodes) taken = taken || done.count(q);
      if (taken) continue;
      const size_t head = *std::min_element(f.nodes.begin(), f.nodes.end());
      for (size_t q : f.nodes)
        if (q != head) done.insert(q);
      gelu[head] = f;
    }
  }

  // `out` (a launch's output so far, written by node `last`) is read by an erf
  // GELU and by nothing else: the activation into *ep, the pattern's nodes
  // done; returns the pattern's last node for the caller to absorb, or -1
  int gelu_pair(const std::string& out, size_t last, Epilogue* ep) {
    if (gelu.empty() || consumers[out] != 2) return -1;
    for (const IO& o : g.outputs)
      if (o.name == out) return -1;
    for (auto& kv : gelu) {
      if (kv.first <= last || kv.second.x != out || done.count(kv.first)) continue;
      ep->act = ACT_GELU;
      done.insert(kv.first);
      return (int)kv.second.last;
    }
    return -1;
  }
  // either decomposed activation behind `out`
  int act_pair(const std::string& out, size_t last, Epilogue* ep) {
    const int mul = hswish_pair(out, last, ep);
    return mul >= 0 ? mul : gelu_pair(out, last, ep);
  }

  // ---- the A/B knobs that change a plan ------------------------------------
  // VSO_ATTN=0: an attention pattern stays its Transpose, MatMul, scale, bias, Softmax and MatMul launches
  static bool attn_enabled() { static const bool on = env_on("VSO_ATTN"); return on; }
  // VSO_HEAD=0: a class head's Resize, channel selection and Equal -> Cast keep their own launches
  static bool head_enabled() { static const bool on = env_on("VSO_HEAD"); return on; }
  // VSO_DECONV_TILE=0: every strided ConvTranspose on k_deconv_direct
  static bool deconv_tile_enabled() { static const bool on = env_on("VSO_DECONV_TILE"); return on; }
  // VSO_DECONV_PAIR=0 / 1: k_deconv_tile<1> (one x phase per workgroup, strided stores) / <2> (both, rows
  // stored contiguous) for every sw == 2 layer; unset: <2> from kDeconvPairMinWgs of its workgroups on
  static long deconv_pair() { static const long v = env_int("VSO_DECONV_PAIR", -1); return v; }
  // VSO_CAT_TAIL=0: every Concat input not written in place is copied
  static bool cat_tail_enabled() { static const bool on = env_on("VSO_CAT_TAIL"); return on; }
  // VSO_GEMM_ACT=0: a Gemm / MatMul's activation as its own launch
  static bool gemm_act_enabled() { static const bool on = env_on("VSO_GEMM_ACT"); return on; }
  // VSO_IR=0: the inverted residual blocks as three launches each
  static bool ir_enabled() { static const bool on = env_on("VSO_IR"); return on; }
  // the bf16x3 form in bf16 / f16 sessions (VSO_IR_B16=0: the f32 form there too)
  static bool ir_b16_enabled() { static const bool on = env_on("VSO_IR_B16"); return on; }
  // VSO_UP_FUSE=0 keeps every Resize a launch of its own
  static bool up_fuse_enabled() { static const bool on = env_on("VSO_UP_FUSE"); return on; }
  // VSO_NORM_PLANE=0: small InstanceNorm planes keep the stats + apply pair
  static bool norm_plane_enabled() { static const bool on = env_on("VSO_NORM_PLANE"); return on; }
  // VSO_THIN=0: 1x1 heads of <= kThinMaxM outputs stay on the MFMA kernels
  static bool thin_enabled() { static const bool on = env_on("VSO_THIN"); return on; }

  // ---- allocations, values, launches ---------------------------------------
  bool fail(const std::string& m) {
    err = m;
    return false;
  }

  template <class T>
  bool dalloc(T** p, size_t bytes) {
    void* q = nullptr;
    const size_t n = std::max<size_t>(bytes, 16);
    if (hipMalloc(&q, n) != hipSuccess) return fail("hipMalloc failed");
    s->allocs.push_back(q);
    s->ranges.push_back(DevRange{(uintptr_t)q, (uintptr_t)q + n, false});
    *p = static_cast<T*>(q);
    return true;
  }
  // a constant's allocation (weights, biases, tables): kernels only read it
  void mark_ro(const void* q) {
    for (DevRange& r : s->ranges)
      if ((uintptr_t)q >= r.lo && (uintptr_t)q < r.hi) r.ro = true;
  }
  // a read-only device copy of `bytes` host bytes
  const void* upload_bytes(const void* src, size_t bytes, const char* what = "constant upload failed") {
    unsigned char* d = nullptr;
    if (!dalloc(&d, bytes)) return nullptr;
    if (bytes && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
      fail(what);
      return nullptr;
    }
    mark_ro(d);
    return d;
  }
  const float* upload_vec(const std::vector<float>& v) {
    return static_cast<const float*>(upload_bytes(v.data(), v.size() * 4));
  }
  // device copy of a constant's float data (cached per Const)
  const float* upload(const Const& c) {
    auto it = dev_consts.find(&c);
    if (it != dev_consts.end()) return it->second;
    const float* d = upload_vec(c.f);
    if (d) dev_consts[&c] = const_cast<float*>(d);
    return d;
  }

  int new_buf(int64_t elems) {
    float* d = nullptr;
    if (!dalloc(&d, (size_t)std::max<int64_t>(elems, 1) * 4)) return -1;
    s->bufs.push_back(d);
    s->buf_elems.push_back(elems);
    return (int)s->bufs.size() - 1;
  }

  Value* val(const std::string& n) {
    if (n.empty()) return nullptr;
    auto it = vals.find(n);
    return it == vals.end() ? nullptr : &it->second;
  }
  float* dptr(const Value& v) { return s->bufs[v.buf]; }
  // a runtime pointer for an operand: its buffer, or its uploaded constant
  const float* operand(Value& v) { return v.is_const ? upload(v.c) : s->bufs[v.buf]; }

  bool set_runtime(const std::string& name, const std::vector<int64_t>& shape, int alias = -1) {
    Value v;
    v.shape = shape;
    v.buf = alias >= 0 ? alias : new_buf(v.numel());
    if (v.buf < 0) return false;
    vals[name] = v;
    return true;
  }
  // a new runtime tensor: its device pointer, or null (err set)
  float* make_out(const std::string& name, const std::vector<int64_t>& shape) {
    return set_runtime(name, shape) ? dptr(vals[name]) : nullptr;
  }
  void set_const(const std::string& name, const Const& c) {
    Value v;
    v.is_const = true;
    v.c = c;
    v.shape = c.dims;
    vals[name] = v;
  }

  template <class T>
  static Region reg(const std::shared_ptr<T>& sp) {
    return Region{std::static_pointer_cast<const void>(sp), sp.get(), sizeof(T)};
  }
  // One launch, `launch(*pp, stream)`.  The parameter block is registered as
  // the launch's region: schedule_lanes finds the launch's dependencies by
  // scanning those bytes for device pointers.
  template <class P, class F>
  void add(const char* name, const std::shared_ptr<P>& pp, F launch) {
    s->launches.push_back(Launch{name, [pp, launch](hipStream_t st) { launch(*pp, st); }, {reg(pp)}});
  }
  // ... of a parameter block the launch list keeps (returned for later patches)
  template <class P, class F>
  std::shared_ptr<P> emit(const char* name, const P& p, F launch) {
    auto pp = std::make_shared<P>(p);
    add(name, pp, launch);
    return pp;
  }
  // `pp` (ConvParams, ResizeParams: `channels` of Ho x Wo) writes `out`; when
  // `out` is a Concat input written in place, plan_concat re-points it there
  template <class P>
  void retarget_on_concat(const std::string& out, const std::shared_ptr<P>& pp, int channels) {
    if (!cat_direct.count(out)) return;
    cat_patch[out].push_back([pp, channels](float* base, int ctot) {
      pp->y = base;
      pp->y_nx = (long)(ctot - channels) * pp->Ho * pp->Wo;
    });
  }

  // ---- graph queries -------------------------------------------------------
  static bool is_act(const std::string& op) {
    return op == "Relu" || op == "Clip" || op == "PRelu" || op == "LeakyRelu" || op == "Sigmoid" || op == "Tanh" ||
           op == "HardSigmoid" || op == "HardSwish" || op == "Gelu";
  }

  // the single node consuming `name`, if exactly one and `name` is no graph output
  int sole_consumer(const std::string& name, size_t after) {
    if (consumers[name] != 1) return -1;
    for (const IO& o : g.outputs)
      if (o.name == name) return -1;
    for (size_t k = after + 1; k < g.nodes.size(); ++k)
      for (const std::string& i : g.nodes[k].in)
        if (i == name) return (int)k;
    return -1;
  }

  int producer(const std::string& name) const {
    for (size_t k = 0; k < g.nodes.size(); ++k)
      for (const std::string& o : g.nodes[k].out)
        if (o == name) return (int)k;
    return -1;
  }

  // activation parameters of an activation node (constants only)
  bool act_of(const Node& nd, Epilogue* ep, int channels) {
    if (nd.op == "Relu") ep->act = ACT_RELU;
    else if (nd.op == "Sigmoid") ep->act = ACT_SIGMOID;
    else if (nd.op == "Tanh") ep->act = ACT_TANH;
    else if (nd.op == "LeakyRelu") { ep->act = ACT_LEAKY; ep->a0 = nd.af("alpha", 0.01f); }
    else if (nd.op == "HardSigmoid") { ep->act = ACT_HSIGMOID; ep->a0 = nd.af("alpha", 0.2f); ep->a1 = nd.af("beta", 0.5f); }
    else if (nd.op == "HardSwish") { ep->act = ACT_HSWISH; ep->a0 = 1.f / 6.f; ep->a1 = 0.5f; }
    else if (nd.op == "Erf") ep->act = ACT_ERF;
    else if (nd.op == "Gelu") {
      const std::string ap = nd.as("approximate", "none");
      if (ap != "none" && ap != "tanh") return false;
      ep->act = ap == "tanh" ? ACT_GELU_TANH : ACT_GELU;
    }
    else if (nd.op == "Clip") {
      float lo = nd.af("min", -INFINITY), hi = nd.af("max", INFINITY);
      if (nd.in.size() > 1 && !nd.in[1].empty()) { Value* v = val(nd.in[1]); if (!v || !v->is_const) return false; lo = v->c.f[0]; }
      if (nd.in.size() > 2 && !nd.in[2].empty()) { Value* v = val(nd.in[2]); if (!v || !v->is_const) return false; hi = v->c.f[0]; }
      ep->act = ACT_CLIP; ep->a0 = lo; ep->a1 = hi;
    } else if (nd.op == "PRelu") {
      Value* sl = val(nd.in[1]);
      if (!sl || !sl->is_const) return false;
      const int64_t n = sl->c.numel();
      if (n != 1 && n != channels) return false;
      // the slope must be per channel under ONNX broadcasting against NCHW:
      // [C,1,1], [1,C,1,1] or one value ([C] aligns with W: left to k_binary)
      const std::vector<int64_t>& sd = sl->c.dims;
      if (n != 1) {
        const size_t r = sd.size();
        if (r < 3 || r > 4 || sd[r - 3] != n) return false;
      }
      ep->act = ACT_PRELU;
      ep->slope = upload(sl->c);
      ep->slope_stride = n == 1 ? 0 : 1;
    } else return false;
    return true;
  }

  // auto_pad SAME_UPPER / SAME_LOWER of a convolution or pool (ConvParams,
  // PoolParams: H, W, kernel, strides, dilations set): pads = {top, left,
  // bottom, right}; false: `ap` is neither
  template <class P>
  static bool same_pads(const std::string& ap, const P& p, int pads[4]) {
    if (ap != "SAME_UPPER" && ap != "SAME_LOWER") return false;
    const int in[2] = {p.H, p.W}, k[2] = {p.kh, p.kw}, st[2] = {p.sh, p.sw}, dl[2] = {p.dh, p.dw};
    for (int d = 0; d < 2; ++d) {
      const int o = (in[d] + st[d] - 1) / st[d];
      const int tot = std::max((o - 1) * st[d] + dl[d] * (k[d] - 1) + 1 - in[d], 0);
      pads[d] = ap == "SAME_UPPER" ? tot / 2 : tot - tot / 2;
      pads[d + 2] = tot - pads[d];
    }
    return true;
  }

  // BatchNormalization `bn` (constant parameters): y = (x - mean) * a + B per
  // channel, a = scale / sqrt(var + epsilon)
  struct BnConsts {
    const Const &scale, &B, &mean, &var;
    double eps;
    double a(int c) const { return scale.f[c] / std::sqrt((double)var.f[c] + eps); }
  };
  BnConsts bn_consts(const Node& bn) {
    return {val(bn.in[1])->c, val(bn.in[2])->c, val(bn.in[3])->c, val(bn.in[4])->c, bn.af("epsilon", 1e-5f)};
  }
  // ... folded into a convolution's output channels [m0, m1): `per` weights each
  void fold_bn(std::vector<float>& wf, std::vector<float>& bias, int64_t per, int m0, int m1, const Node& bn) {
    const BnConsts b = bn_consts(bn);
    for (int m = m0; m < m1; ++m) {
      const double a = b.a(m);
      for (int64_t k = 0; k < per; ++k) wf[m * per + k] = (float)(wf[m * per + k] * a);
      bias[m] = (float)((bias[m] - b.mean.f[m]) * a + b.B.f[m]);
    }
  }

  // ---- the inverted residual block (vso_ir.hip) ----------------------------
  // A constant conv's geometry: 1x1 / stride 1 / unpadded / undilated, or the
  // 3x3 depthwise of a MobileNetV2 block (pads 1, stride 1 or 2)
  bool conv_attrs(const Node& c, int k, int* stride, int* group) {
    if (c.as("auto_pad", "NOTSET") != "NOTSET") return false;
    const std::vector<int64_t> st = c.ais("strides"), dl = c.ais("dilations"), pd = c.ais("pads");
    for (int64_t v : dl) if (v != 1) return false;
    const int sh = st.size() > 0 ? (int)st[0] : 1, sw = st.size() > 1 ? (int)st[1] : 1;
    if (sh != sw) return false;
    for (int64_t v : pd) if (v != (k == 3 ? 1 : 0)) return false;
    if (k == 3 && pd.size() != 4) return false;
    *stride = sh;
    *group = (int)c.ai("group", 1);
    return true;
  }

  // The MobileNetV2 inverted residual starting at Conv ni: 1x1 expand -> Clip
  // -> 3x3 depthwise (stride 1 / 2) -> Clip -> 1x1 project [-> Add of the
  // block's input], each value consumed by the next node only
  struct IrBlock {
    int k1, k2, k3, k4, k5;  // the Clip, depthwise, Clip, project and Add nodes (k5: when res)
    Value *x, *w1, *wd, *w2;
    std::vector<float> b1, bd, b2;
    Epilogue c1{}, c2{};
    int sd;  // the depthwise stride
    bool res;
    std::string out;
  };
  bool match_ir(size_t ni, IrBlock* b) {
    const Node& ex = g.nodes[ni];
    if (ibn.count(ni) || ex.in.size() < 2) return false;
    // an input that is a depthwise output left to its 1x1 consumer (pending_dw:
    // no launch writes it) is computed by plan_conv's fused form, not here
    if (pending_dw.count(ex.in[0])) return false;
    Value *x = b->x = val(ex.in[0]), *w1 = b->w1 = val(ex.in[1]);
    if (!x || x->is_const || x->shape.size() != 4 || !w1 || !w1->is_const || w1->c.dims.size() != 4) return false;
    int s1, g1;
    if (!conv_attrs(ex, 1, &s1, &g1) || s1 != 1 || g1 != 1 || w1->c.dims[2] != 1 || w1->c.dims[3] != 1) return false;
    const int CIN = (int)x->shape[1], HID = (int)w1->c.dims[0];
    if (w1->c.dims[1] != CIN) return false;
    const int k1 = b->k1 = sole_consumer(ex.out[0], ni);
    if (k1 < 0 || g.nodes[k1].op != "Clip") return false;
    const int k2 = b->k2 = sole_consumer(g.nodes[k1].out[0], k1);
    if (k2 < 0 || g.nodes[k2].op != "Conv" || g.nodes[k2].in[0] != g.nodes[k1].out[0]) return false;
    const int k3 = b->k3 = sole_consumer(g.nodes[k2].out[0], k2);
    if (k3 < 0 || g.nodes[k3].op != "Clip") return false;
    const int k4 = b->k4 = sole_consumer(g.nodes[k3].out[0], k3);
    if (k4 < 0 || g.nodes[k4].op != "Conv" || g.nodes[k4].in[0] != g.nodes[k3].out[0]) return false;
    const Node &dw = g.nodes[k2], &pj = g.nodes[k4];
    Value *wd = b->wd = val(dw.in[1]), *w2 = b->w2 = val(pj.in[1]);
    int gd, s2, g2;
    if (!wd || !wd->is_const || wd->c.dims.size() != 4 || !conv_attrs(dw, 3, &b->sd, &gd) ||
        (b->sd != 1 && b->sd != 2) || gd != HID || wd->c.dims[0] != HID || wd->c.dims[1] != 1 ||
        wd->c.dims[2] != 3 || wd->c.dims[3] != 3)
      return false;
    if (!w2 || !w2->is_const || w2->c.dims.size() != 4 || !conv_attrs(pj, 1, &s2, &g2) || s2 != 1 || g2 != 1 ||
        w2->c.dims[1] != HID || w2->c.dims[2] != 1 || w2->c.dims[3] != 1)
      return false;
    const int COUT = (int)w2->c.dims[0];
    auto bias_of = [&](const Node& c, int m, std::vector<float>* bv) {
      bv->assign(m, 0.f);
      if (c.in.size() < 3 || c.in[2].empty()) return true;
      Value* v = val(c.in[2]);
      if (!v || !v->is_const || v->c.numel() != m) return false;
      *bv = v->c.f;
      return true;
    };
    if (!bias_of(ex, HID, &b->b1) || !bias_of(dw, HID, &b->bd) || !bias_of(pj, COUT, &b->b2)) return false;
    if (!act_of(g.nodes[k1], &b->c1, HID) || !act_of(g.nodes[k3], &b->c2, HID)) return false;
    // the residual: an Add of the project's output and the block's input
    b->out = pj.out[0];
    b->k5 = sole_consumer(b->out, k4);
    b->res = false;
    if (b->k5 >= 0 && g.nodes[b->k5].op == "Add") {
      const Node& ad = g.nodes[b->k5];
      const std::string& other = ad.in[0] == b->out ? ad.in[1] : ad.in[0];
      // a strided residual find_residual_fusions left to the project's epilogue (its MaxPool / Pad
      // nodes are done, nothing writes `other`): the generic plan, whose plan_conv reads the pool's input
      if (res_fuse.count(other)) return false;
      if (other == ex.in[0] && ad.in[0] != ad.in[1] && b->sd == 1 && CIN == COUT) {
        b->res = true;
        b->out = ad.out[0];
      }
    }
    return !cat_direct.count(b->out) && !cat_direct.count(pj.out[0]);  // (written into a Concat: the generic path)
  }

  // ... as one k_ir launch.  1: planned (the other nodes marked done), 0: not
  // this pattern / no kernel for its shape, -1: an error.
  int try_plan_ir(size_t ni) {
    IrBlock b;
    if (!ir_enabled() || !match_ir(ni, &b)) return 0;
    const std::vector<int64_t>& xs = b.x->shape;
    const int N = (int)xs[0], CIN = (int)xs[1], H = (int)xs[2], W = (int)xs[3];
    const int HID = (int)b.w1->c.dims[0], COUT = (int)b.w2->c.dims[0], sd = b.sd;
    const int Ho = (H + 2 - 3) / sd + 1, Wo = (W + 2 - 3) / sd + 1;
    IrParams p{};
    p.N = N; p.CIN = CIN; p.H = H; p.W = W; p.HID = HID; p.COUT = COUT; p.Ho = Ho; p.Wo = Wo;
    p.stride = sd; p.res = b.res ? 1 : 0;
    p.lo1 = b.c1.a0; p.hi1 = b.c1.a1; p.lo2 = b.c2.a0; p.hi2 = b.c2.a1;
    p.b16 = s->conv_precision != PREC_F32 && ir_b16_enabled() ? 1 : 0;
    ir_tiles(Ho, Wo, &p.tiles_x, &p.tiles);
    // slices of the hidden channels: about two workgroups per CU (512; VSO_IR_WGS:
    // 256 measured 1.445 against 1.424 ms on MODNet batch 8 bf16, profiles/r05f)
    // over the tiles and slices, whole 16-channel chunks per slice (b16: whole
    // chunk pairs, and the slice's weights within the LDS budget)
    static const long wgs = std::max(1L, env_int("VSO_IR_WGS", 512));
    static const int probe = (int)env_int("VSO_IR_PROBE", 0);
    p.probe = probe;
    static const bool wave_form = env_off("VSO_IR_WAVE");
    p.wv = p.b16 && wave_form && CIN <= 64 ? 1 : 0;
    const int nch = HID / 16;
    // b16: about 6 chunks per slice, at least 256 workgroups (VSO_IR_CPS; 0:
    // the VSO_IR_WGS target alone) — MODNet batch 8 bf16 1407.5 us of kernel
    // time against 1411 (4), 1415 (8), 1421 (the 512-workgroup target),
    // profiles/r05i
    static const int cps_target = (int)env_int("VSO_IR_CPS", 6);
    if (p.b16 && (HID % 16 != 0 || !ir_slab_plan(&p, wgs, cps_target))) return 0;
    if (!ir_supported(p)) return 0;
    if (!p.b16) {
      const long wg0 = (long)N * p.tiles;
      int ks = (int)std::min<long>(nch, std::max<long>(1, (wgs + wg0 / 2) / wg0));
      p.cps = (nch + ks - 1) / ks;
      p.ks = (nch + p.cps - 1) / p.cps;
    }
    p.pstr = ir_pstr(sd);
    // weights: the expand / project as stored ([out][in]), the depthwise tap-major
    const std::vector<float>&w1 = b.w1->c.f, &w2 = b.w2->c.f;
    std::vector<float> wdt((size_t)9 * HID);
    for (int h = 0; h < HID; ++h)
      for (int k = 0; k < 9; ++k) wdt[(size_t)k * HID + h] = b.wd->c.f[(size_t)h * 9 + k];
    const std::string& in0 = g.nodes[ni].in[0];
    flush_input(in0);
    flush_norm(in0);
    p.x = dptr(*b.x);
    p.w1 = upload_vec(w1);
    p.b1 = upload_vec(b.b1);
    p.wdw = upload_vec(wdt);
    p.bdw = upload_vec(b.bd);
    p.w2 = upload_vec(w2);
    p.b2 = upload_vec(b.b2);
    if (!p.w1 || !p.b1 || !p.wdw || !p.bdw || !p.w2 || !p.b2) return -1;
    if (p.b16) {
      std::vector<unsigned char> slab;
      ir_slab_build(p, w1.data(), b.b1.data(), wdt.data(), b.bd.data(), w2.data(), &slab);
      p.slab = static_cast<const unsigned char*>(upload_bytes(slab.data(), slab.size()));
      if (!p.slab) return -1;
    }
    if (p.ks > 1 && !dalloc(&p.part, (size_t)p.ks * N * COUT * Ho * Wo * 4)) return -1;
    if (!(p.y = make_out(b.out, {N, COUT, Ho, Wo}))) return -1;
    auto pp = emit(ir_kernel_name(p), p, launch_ir);
    if (p.ks > 1) add("void vso::k_ir_reduce(vso::IrParams)", pp, launch_ir_reduce);
    for (int k : {b.k1, b.k2, b.k3, b.k4}) done.insert((size_t)k);
    if (b.res) done.insert((size_t)b.k5);
    s->ir_blocks++;
    return 1;
  }

  // ---- Conv ----------------------------------------------------------------
  // A Conv node with what its launch absorbs
  struct ConvPlan {
    ConvParams p{};
    std::vector<float> wf, bias;  // weights and bias, BatchNormalization folded in
    bool has_bias = false;
    std::vector<int64_t> oshape;
    std::string out;              // the value the launch writes: the last absorbed node's output
    size_t last;                  // that node
    const IbnFuse* ib = nullptr;  // the IBNorm this Conv heads
  };

  // geometry and attribute checks: c->p's sizes, c->wf, c->bias
  bool conv_geometry(const Node& nd, ConvPlan* c) {
    Value* x = val(nd.in[0]);
    Value* w = val(nd.in[1]);
    Value* b = nd.in.size() > 2 ? val(nd.in[2]) : nullptr;
    if (!w || !w->is_const) return fail("Conv '" + nd.name + "': weights must be constant");
    if (x->shape.size() != 4 || w->c.dims.size() != 4) return fail("Conv '" + nd.name + "': 2D only");
    ConvParams& p = c->p;
    p.N = (int)x->shape[0]; p.C = (int)x->shape[1]; p.H = (int)x->shape[2]; p.W = (int)x->shape[3];
    p.M = (int)w->c.dims[0]; p.Cg = (int)w->c.dims[1]; p.kh = (int)w->c.dims[2]; p.kw = (int)w->c.dims[3];
    p.G = (int)nd.ai("group", 1);
    if (p.G < 1 || p.C != p.Cg * p.G || p.M % p.G) return fail("Conv '" + nd.name + "': channel/group mismatch");
    p.Mg = p.M / p.G;
    std::vector<int64_t> st = nd.ais("strides"), dl = nd.ais("dilations"), pd = nd.ais("pads");
    // (absent, or one value per axis / per side: a shorter list would leave an axis at its default unnoticed)
    if (!st.empty() && st.size() != 2) return fail("Conv '" + nd.name + "': strides must have 2 values");
    if (!dl.empty() && dl.size() != 2) return fail("Conv '" + nd.name + "': dilations must have 2 values");
    if (!pd.empty() && pd.size() != 4) return fail("Conv '" + nd.name + "': pads must have 4 values");
    p.sh = st.empty() ? 1 : (int)st[0]; p.sw = st.empty() ? 1 : (int)st[1];
    p.dh = dl.empty() ? 1 : (int)dl[0]; p.dw = dl.empty() ? 1 : (int)dl[1];
    if (p.sh < 1 || p.sw < 1 || p.dh < 1 || p.dw < 1)
      return fail("Conv '" + nd.name + "': strides and dilations must be positive");
    int pads[4] = {0, 0, 0, 0};  // top, left, bottom, right
    for (size_t k = 0; k < pd.size(); ++k) pads[k] = (int)pd[k];
    const std::string ap = nd.as("auto_pad", "NOTSET");
    if (!same_pads(ap, p, pads) && ap == "VALID") pads[0] = pads[1] = pads[2] = pads[3] = 0;
    p.pt = pads[0]; p.pl = pads[1];
    p.Ho = (p.H + pads[0] + pads[2] - p.dh * (p.kh - 1) - 1) / p.sh + 1;
    p.Wo = (p.W + pads[1] + pads[3] - p.dw * (p.kw - 1) - 1) / p.sw + 1;
    if (p.Ho < 1 || p.Wo < 1) return fail("Conv '" + nd.name + "': empty output");
    c->oshape = {p.N, p.M, p.Ho, p.Wo};
    c->wf = w->c.f;
    c->bias.assign(p.M, 0.f);
    if (b) {
      if (!b->is_const || b->c.numel() != p.M) return fail("Conv '" + nd.name + "': bias must be constant [M]");
      c->bias = b->c.f;
      c->has_bias = true;
    }
    return true;
  }

  // `node` (absorbed) now ends the launch
  void absorb(ConvPlan* c, int node, int* next) {
    done.insert((size_t)node);
    c->out = g.nodes[node].out[0];
    c->last = (size_t)node;
    *next = sole_consumer(c->out, c->last);
  }

  // epilogue absorption: BatchNormalization -> residual Add -> activation (an
  // IBNorm: its BatchNorm half and Relu), while each value has one consumer
  bool conv_absorb(size_t ni, ConvPlan* c) {
    ConvParams& p = c->p;
    Epilogue& ep = p.ep;
    c->out = g.nodes[ni].out[0];
    c->last = ni;
    int c1 = sole_consumer(c->out, c->last);
    const int64_t per = (int64_t)p.Cg * p.kh * p.kw;
    const auto ib = ibn.find(ni);
    if (ib != ibn.end()) {  // BN folded into channels < nb, Relu there; the InstanceNorm after the launch
      const IbnFuse& f = ib->second;
      c->ib = &f;
      fold_bn(c->wf, c->bias, per, 0, f.nb, g.nodes[f.bn]);
      c->has_bias = true;
      if (f.relu >= 0) {
        ep.act = ACT_RELU;
        ep.act_c_end = f.nb;
      }
      c->out = f.out;
      c1 = -1;
    }
    if (c1 >= 0 && g.nodes[c1].op == "BatchNormalization") {
      const Node& bn = g.nodes[c1];
      Value *sc = val(bn.in[1]), *bb = val(bn.in[2]), *mu = val(bn.in[3]), *vr = val(bn.in[4]);
      if (sc && bb && mu && vr && sc->is_const && bb->is_const && mu->is_const && vr->is_const &&
          sc->c.numel() == p.M) {
        fold_bn(c->wf, c->bias, per, 0, p.M, bn);
        c->has_bias = true;
        absorb(c, c1, &c1);
      }
    }
    if (c1 >= 0 && g.nodes[c1].op == "Add") {
      const Node& ad = g.nodes[c1];
      const std::string& other = ad.in[0] == c->out ? ad.in[1] : ad.in[0];
      auto rf = res_fuse.find(other);
      if (rf != res_fuse.end()) {
        // the epilogue addresses the source per image, channel and output pixel: an Add that broadcasts
        // its operand (one image for the batch, one pixel for the plane) is not that — the MaxPool / Pad
        // get their launches after all (they stay `done`: the walk does not plan them again)
        const int mode = rf->second.mode;
        Value* src = val(rf->second.src);
        if (!src || src->is_const || src->shape.size() != 4 || src->shape[0] != p.N || src->shape[1] > p.M ||
            (mode == 1 && (src->shape[2] != p.Ho || src->shape[3] != p.Wo)) ||
            (mode == 2 && (src->shape[2] / 2 != p.Ho || src->shape[3] / 2 != p.Wo))) {
          for (int k : {rf->second.pool_node, rf->second.pad_node})
            if (k >= 0 && !plan_node((size_t)k)) return false;
          res_fuse.erase(rf);
          rf = res_fuse.end();
        }
      }
      Value* o = val(rf != res_fuse.end() ? rf->second.src : other);
      if (rf != res_fuse.end()) {  // the strided residual: the MaxPool / Pad computed here
        const int mode = rf->second.mode;
        ep.res = dptr(*o);
        ep.res_mode = mode;
        ep.res_c = (int)o->shape[1];
        ep.res_h = (int)o->shape[2];
        ep.res_w = (int)o->shape[3];
        ep.out_c = p.M;
        ep.out_hw = p.Ho * p.Wo;
        ep.out_w = p.Wo;
        absorb(c, c1, &c1);
      } else if (o && !o->is_const && o->shape == c->oshape && ad.in[0] != ad.in[1]) {
        ep.res = dptr(*o);
        absorb(c, c1, &c1);
      }
    }
    if (c1 >= 0 && is_act(g.nodes[c1].op) && act_of(g.nodes[c1], &ep, p.M)) absorb(c, c1, &c1);
    else if (c1 < 0 && !c->ib && ep.act == ACT_NONE) {
      const int mul = act_pair(c->out, c->last, &ep);
      if (mul >= 0) absorb(c, mul, &c1);
    }
    return err.empty();
  }

  // `out`'s sole consumer is a Conv k_conv_thin runs (thin_conv_fits, C <= kThinMaxC)
  static constexpr int kThinMaxC = 256;
  bool feeds_thin(const std::string& out, size_t last) {
    const int c = sole_consumer(out, last);
    if (c < 0) return false;
    const Node& cv = g.nodes[c];
    if (cv.op != "Conv" || cv.in.empty() || cv.in[0] != out || cv.in.size() < 2) return false;
    Value* w = val(cv.in[1]);
    if (!w || !w->is_const || w->c.dims.size() != 4) return false;
    const std::vector<int64_t>& d = w->c.dims;
    if (d[0] > kThinMaxM || d[1] > kThinMaxC || d[2] != 1 || d[3] != 1 || cv.ai("group", 1) != 1) return false;
    for (int64_t v : cv.ais("strides")) if (v != 1) return false;
    for (int64_t v : cv.ais("pads")) if (v != 0) return false;
    const std::string ap = cv.as("auto_pad", "NOTSET");
    return ap == "NOTSET" || ap == "VALID";
  }

  // output channels of the sole Conv consuming `out` (its weights' dims[0]), or 0
  int consumer_out_channels(const std::string& out, size_t last) {
    const int c = sole_consumer(out, last);
    if (c < 0 || g.nodes[c].op != "Conv" || g.nodes[c].in.size() < 2) return 0;
    Value* w = val(g.nodes[c].in[1]);
    return (w && w->is_const && !w->c.dims.empty()) ? (int)w->c.dims[0] : 0;
  }

  // The output of a depthwise conv feeds exactly one Conv, 1x1 / stride 1 /
  // unpadded / ungrouped, on all its channels: the pair runs as k_conv_dwpw.
  bool feeds_pointwise(const std::string& out, size_t last, int channels) {
    const int c = sole_consumer(out, last);
    if (c < 0 || g.nodes[c].op != "Conv" || g.nodes[c].in.empty() || g.nodes[c].in[0] != out) return false;
    const Node& pw = g.nodes[c];
    Value* w = val(pw.in[1]);
    if (!w || !w->is_const || w->c.dims.size() != 4 || w->c.dims[1] != channels || w->c.dims[2] != 1 ||
        w->c.dims[3] != 1 || pw.ai("group", 1) != 1 || pw.as("auto_pad", "NOTSET") != "NOTSET")
      return false;
    for (int64_t v : pw.ais("strides")) if (v != 1) return false;
    for (int64_t v : pw.ais("pads")) if (v != 0) return false;
    for (int64_t v : pw.ais("dilations")) if (v != 1) return false;
    return true;
  }

  // a depthwise conv whose 1x1 consumer computes it (k_conv_pw / k_conv_dwpw): no launch
  bool defer_depthwise(const ConvPlan& c) {
    const ConvParams& p = c.p;
    // (k_conv_pw stages the pair's channels in chunks: any count for a 3x3 / 5x5
    // depthwise on enough pixels; k_conv_dwpw, the rest, holds all of them in LDS)
    const int pw_m = consumer_out_channels(c.out, c.last);
    // (pw_pair_fits: pw_kernel's own test, its 32-bit offset limits included —
    // a pair it declined would fall to k_conv_dwpw, whose LDS holds kDwPwMaxC)
    const bool pw_dw = p.kh == p.kw && (p.kh == 3 || p.kh == 5) && pw_m > 0 &&
                       pw_pair_fits(p.N, p.C, (long)p.H * p.W, (long)p.Ho * p.Wo, pw_m);
    return p.G == p.C && p.G == p.M && !p.ep.res && !c.ib && (pw_dw || p.C <= kDwPwMaxC) &&
           feeds_pointwise(c.out, c.last, p.M);
  }

  bool plan_conv(size_t ni, const Node& nd, Ins&) {
    const std::string& in0 = nd.in[0];
    // a deferred Concat copy into this Conv's input: only a dense 3x3 / 5x5
    // convolution (plan_conv_dense, which takes it or flushes) may take it;
    // every other plan reads the whole concatenation
    if (cat_tail.count(in0)) {
      Value* w = nd.in.size() > 1 ? val(nd.in[1]) : nullptr;
      const bool dense = w && w->shape.size() == 4 && nd.ai("group", 1) == 1 && w->shape[2] == w->shape[3] &&
                         (w->shape[2] == 3 || w->shape[2] == 5);
      if (!dense && !flush_tail(in0)) return false;
    }
    if (const int rc = try_plan_ir(ni)) return rc > 0;
    ConvPlan c;
    if (!conv_geometry(nd, &c) || !conv_absorb(ni, &c)) return false;
    ConvParams& p = c.p;
    p.w = upload_vec(c.wf);
    p.ep.bias = c.has_bias ? upload_vec(c.bias) : nullptr;
    if (!p.w || (c.has_bias && !p.ep.bias)) return false;
    p.x = dptr(*val(in0));
    if (!(p.y = make_out(c.out, c.oshape))) return false;
    if (defer_depthwise(c)) {
      flush_input(in0);
      pending_dw[c.out] = {p.x, DwPre{p.w, p.H, p.W, p.kh, p.kw, p.sh, p.sw, p.dh, p.dw, p.pt, p.pl, p.ep}};
      return true;
    }
    auto pre = pending_dw.find(in0);
    if (pre != pending_dw.end()) {
      if (p.G != 1 || p.kh != 1 || p.kw != 1 || p.sh != 1 || p.sw != 1 || p.pt || p.pl || p.Ho != p.H || p.Wo != p.W)
        return fail("Conv '" + nd.name + "': internal: fused depthwise producer");
      p.x = pre->second.first;
      p.pre = pre->second.second;
      pending_dw.erase(pre);  // (its sole consumer: taken)
    }
    if (!c.ib && thin_conv_fits(p) && p.C <= kThinMaxC && thin_enabled()) return plan_conv_thin(in0, c);
    flush_norm(in0);  // (a pending InstanceNorm apply step: not taken here)
    if (!plan_conv_dense(in0, c, s->conv_precision)) return false;
    if (!c.ib) return true;
    const Node& inn = g.nodes[c.ib->inorm];
    const std::string* direct = cat_direct.count(c.out) ? &c.out : nullptr;
    // a thin 1x1 consumer normalises its input itself: statistics only here
    const bool defer = !direct && thin_enabled() && feeds_thin(c.out, c.last);
    return plan_norm(p.y, p.y, p.N, p.M - c.ib->nb, c.ib->nb, p.M, (int64_t)p.Ho * p.Wo, inn, val(inn.in[1]),
                     val(inn.in[2]), c.ib->relu >= 0 ? ACT_RELU : ACT_NONE, direct, defer ? &c.out : nullptr);
  }

  // k_conv_thin (a matte / logit head: memory bound, on the VALU); its input's
  // InstanceNorm apply step, when left pending, folded into the loads
  bool plan_conv_thin(const std::string& in0, const ConvPlan& c) {
    std::shared_ptr<NormParams> norm;
    auto nt = norm_pending.find(in0);
    if (nt != norm_pending.end()) {
      norm = nt->second;
      norm_pending.erase(nt);
    }
    flush_input(in0);  // (a pending Resize, or a Concat's pending upsampled inputs)
    auto pp = std::make_shared<ConvParams>(c.p);
    std::vector<Region> io{reg(pp)};
    if (norm) io.push_back(reg(norm));
    s->launches.push_back(
        Launch{conv_thin_name(c.p.M), [pp, norm](hipStream_t st) { launch_conv_thin(*pp, norm.get(), st); }, io});
    retarget_on_concat(c.out, pp, c.p.M);
    return true;
  }

  // k_conv_tile where it has a shape for the convolution (with a 2x upsample
  // of its input, or of one Concat input, computed while staging, and a
  // Concat's tail read in place), else the generic kernels (launch_conv)
  static constexpr double kTileMinMacs = 8e6;  // f32: smaller convs keep k_conv_small / k_conv_gemm
  // (prec: the session's conv_precision; PREC_F32 for a lowered ConvTranspose)
  bool plan_conv_dense(const std::string& in0, const ConvPlan& c, int prec) {
    const ConvParams& p = c.p;
    ConvTileShape ts{};
    const double macs = (double)p.N * p.M * p.Ho * p.Wo * p.Cg * p.kh * p.kw;
    const bool tile = !p.pre.w && conv_tile_shape(p, prec, &ts) && (prec != PREC_F32 || macs >= kTileMinMacs);
    std::vector<UpRange> ups;
    if (up_pending.count(in0)) ups.push_back({in0, 0, p.C});
    else if (cat_up.count(in0)) ups = cat_up[in0];
    const ResizeParams* up = nullptr;
    // (one output-channel tile of at most 32 only: each tile would interpolate
    // the whole input again, and at 64 output channels the interpolation
    // measured slower than the Resize's own launch, MODNet 288x512 b8 bf16)
    static const bool up_bm64 = env_off("VSO_UP_BM64");  // (A/B knob: 64-channel upsample tiles)
    if (tile && ups.size() == 1 && ts.s == 1 && (ts.ks == 3 || ts.ks == 5) && ts.Mp == ts.bm &&
        (ts.bm <= 32 || up_bm64) &&
        ts.prec != PREC_F32 && ups[0].c0 % 32 == 0 && ups[0].c1 % 32 == 0 && up_fuse_enabled()) {
      ConvTileShape tu{};
      tu.up = 1;
      if (conv_tile_shape(p, prec, &tu)) {
        up = up_pending[ups[0].name].get();
        ts = tu;
      }
    }
    for (const UpRange& u : ups)
      if (!up || u.name != ups[0].name) flush_up(u.name);
    if (!tile) {
      if (!flush_tail(in0)) return false;
      auto pp = emit(conv_kernel_name(p), p, [](const ConvParams& q, hipStream_t st) { launch_conv(q, st, nullptr); });
      retarget_on_concat(c.out, pp, p.M);
      return true;
    }
    const CatTail* tail = nullptr;
    auto ct = cat_tail.find(in0);
    if (ct != cat_tail.end() && ct->second.c0 + ct->second.C == p.C && ct->second.c0 % 32 == 0 &&
        (!up || ct->second.c0 >= ups[0].c1))
      tail = &ct->second;
    else if (!flush_tail(in0))
      return false;
    if (!plan_conv_tile(c, ts, up, up ? ups[0].c0 : 0, up ? ups[0].c1 : 0, tail)) return false;
    if (tail) cat_tail.erase(in0);
    if (up) up_pending.erase(ups[0].name);
    return true;
  }

  // A dense convolution on k_conv_tile (vso_conv.hip): weights (BatchNorm
  // folded) packed [tap][Mp][Cp] in the operand type, zero padded; a
  // partial-sum buffer when the channel chunks are split over workgroups.
  bool plan_conv_tile(const ConvPlan& c, const ConvTileShape& ts, const ResizeParams* up, int up_c0, int up_c1,
                      const CatTail* tail) {
    const ConvParams& p = c.p;
    const int taps = p.kh * p.kw;
    const size_t n = (size_t)taps * ts.Mp * ts.Cp;
    ConvTileParams tp{};
    tp.c = p;
    tp.Mp = ts.Mp; tp.Cp = ts.Cp; tp.tiles_x = ts.tiles_x; tp.ksplit = ts.ksplit; tp.cps = ts.cps;
    static const int qskip = (int)env_int("VSO_CONV_QSKIP", 1);
    tp.qskip = qskip;
    static const int xcd = (int)env_int("VSO_CONV_XCD", 1);
    tp.xcd = xcd;
    if (tail) {
      tp.x2 = tail->x;
      tp.x2_c0 = tail->c0;
      tp.x2_C = tail->C;
    }
    tp.tiles = ts.tiles; tp.mtiles = ts.Mp / ts.bm;
    if (up) {
      tp.up = up->x;
      tp.up_H = up->H; tp.up_W = up->W;
      tp.up_c0 = up_c0; tp.up_c1 = up_c1;
    }
    // w[tap][m][c] of the packed layout <- the node's [m][c][tap]
    auto pack = [&](auto* w, auto conv) {
      for (int tap = 0; tap < taps; ++tap)
        for (int m = 0; m < p.M; ++m)
          for (int ch = 0; ch < p.C; ++ch)
            w[((size_t)tap * ts.Mp + m) * ts.Cp + ch] = conv(c.wf[((size_t)m * p.C + ch) * taps + tap]);
    };
    if (ts.prec == PREC_F32) {
      std::vector<float> w(n, 0.f);
      pack(w.data(), [](float v) { return v; });
      tp.wp = upload_bytes(w.data(), n * 4, "conv weight upload failed");
    } else {
      std::vector<uint16_t> w(n, 0);
      if (ts.prec == PREC_BF16) pack(w.data(), [](float v) { return float_to_bf16(v); });
      else pack(w.data(), [](float v) { return float_to_half_bits(v); });
      tp.wp = upload_bytes(w.data(), n * 2, "conv weight upload failed");
    }
    if (!tp.wp) return false;
    if (ts.ksplit > 1) {
      const size_t blocks = (size_t)p.N * (ts.Mp / ts.bm) * ts.tiles;
      // partial tiles in accumulator order: per output block and split, 256 threads x bm/16 x th*tw/64 f4
      const size_t per = (size_t)256 * (ts.bm / 16) * (ts.th * ts.tw / 64) * 16;
      if (!dalloc(&tp.part, blocks * ts.ksplit * per) || !dalloc(&tp.counters, blocks * 4))
        return false;
      if (hipMemset(tp.counters, 0, blocks * 4) != hipSuccess) return fail("hipMemset failed");
    }
    auto tpp = emit(conv_tile_name(ts), tp,
                    [ts](const ConvTileParams& q, hipStream_t st) { launch_conv_tile(q, ts, st); });
    retarget_on_concat(c.out, std::shared_ptr<ConvParams>(tpp, &tpp->c), p.M);
    s->tile_convs++;
    return true;
  }

  // ---- ConvTranspose -------------------------------------------------------
  // Geometry of a ConvTranspose node (include/vso.h: the attribute table) into
  // the ConvPlan of the stride-1 Conv it would equal at stride 1 — weights
  // [M][Cg][kh][kw], flipped in both spatial axes, C and M exchanged within
  // each group, pads d (k - 1) - pads — with the node's strides in *sh / *sw
  // (c->p.sh / sw stay 1: conv_absorb and a lowered Conv read the plan).
  bool deconv_geometry(const Node& nd, Ins& in, ConvPlan* c, int* sh, int* sw) {
    const std::string who = "ConvTranspose '" + nd.name + "'";
    Value *x = in[0], *w = in.size() > 1 ? in[1] : nullptr, *b = in.size() > 2 ? in[2] : nullptr;
    if (!w || !w->is_const) return fail(who + ": weights must be constant");
    if (x->shape.size() != 4 || w->c.dims.size() != 4) return fail(who + ": 2D only");
    ConvParams& p = c->p;
    p.N = (int)x->shape[0]; p.C = (int)x->shape[1]; p.H = (int)x->shape[2]; p.W = (int)x->shape[3];
    p.G = (int)nd.ai("group", 1);
    p.Mg = (int)w->c.dims[1]; p.kh = (int)w->c.dims[2]; p.kw = (int)w->c.dims[3];
    if (p.G < 1 || w->c.dims[0] != p.C || p.C % p.G) return fail(who + ": channel/group mismatch");
    p.Cg = p.C / p.G;
    p.M = p.Mg * p.G;
    const std::vector<int64_t> st = nd.ais("strides"), dl = nd.ais("dilations"), pd = nd.ais("pads"),
                               op = nd.ais("output_padding"), osz = nd.ais("output_shape");
    if (!st.empty() && st.size() != 2) return fail(who + ": strides must have 2 values");
    if (!dl.empty() && dl.size() != 2) return fail(who + ": dilations must have 2 values");
    if (!op.empty() && op.size() != 2) return fail(who + ": output_padding must have 2 values");
    if (!pd.empty() && pd.size() != 4) return fail(who + ": pads must have 4 values");
    if (!osz.empty() && osz.size() != 2) return fail(who + ": output_shape must have 2 values");
    const int64_t in_[2] = {p.H, p.W}, k[2] = {p.kh, p.kw};
    int64_t s[2], d[2], opad[2], pb[2], pe[2], out[2];
    const std::string ap = nd.as("auto_pad", "NOTSET");
    if (ap != "NOTSET" && ap != "VALID" && ap != "SAME_UPPER" && ap != "SAME_LOWER")
      return fail(who + ": auto_pad " + ap);
    for (int a = 0; a < 2; ++a) {
      s[a] = st.empty() ? 1 : st[a];
      d[a] = dl.empty() ? 1 : dl[a];
      opad[a] = op.empty() ? 0 : op[a];
      if (s[a] < 1 || d[a] < 1) return fail(who + ": strides and dilations must be positive");
      if (s[a] > 1024 || d[a] > 1024 || k[a] > 1024) return fail(who + ": strides, dilations and kernels up to 1024 only");
      if (opad[a] < 0 || opad[a] >= std::max(s[a], d[a]))
        return fail(who + ": output_padding must be below max(stride, dilation)");
      const int64_t full = s[a] * (in_[a] - 1) + opad[a] + (k[a] - 1) * d[a] + 1;  // the unpadded output
      const bool same = ap == "SAME_UPPER" || ap == "SAME_LOWER";
      if (!osz.empty() || same) {
        // ONNX's ConvTranspose text: the total padding from the wanted size, then
        // split — SAME_UPPER: total / 2 at the beginning; otherwise at the end
        const int64_t total = full - (osz.empty() ? in_[a] * s[a] : osz[a]);
        if (total < 0) return fail(who + ": the output size asks for negative pads");
        pb[a] = ap == "SAME_UPPER" ? total / 2 : total - total / 2;
        pe[a] = total - pb[a];
      } else {
        pb[a] = pd.empty() || ap == "VALID" ? 0 : pd[a];
        pe[a] = pd.empty() || ap == "VALID" ? 0 : pd[a + 2];
        if (pb[a] < 0 || pe[a] < 0) return fail(who + ": pads must not be negative");
      }
      out[a] = full - pb[a] - pe[a];
      if (out[a] < 1) return fail(who + ": empty output");
    }
    // (the kernels' plane and tensor offsets are int where the neighbouring convolution kernels' are)
    if ((int64_t)p.N * p.M * out[0] * out[1] >= (1LL << 31) || x->numel() >= (1LL << 31))
      return fail(who + ": tensors below 2^31 elements only");
    *sh = (int)s[0]; *sw = (int)s[1];
    p.sh = p.sw = 1;
    p.dh = (int)d[0]; p.dw = (int)d[1];
    p.pt = (int)(d[0] * (k[0] - 1) - pb[0]);
    p.pl = (int)(d[1] * (k[1] - 1) - pb[1]);
    p.Ho = (int)out[0]; p.Wo = (int)out[1];
    c->oshape = {p.N, p.M, p.Ho, p.Wo};
    const int taps = p.kh * p.kw;
    c->wf.assign((size_t)p.M * p.Cg * taps, 0.f);
    for (int gi = 0; gi < p.G; ++gi)
      for (int ch = 0; ch < p.Cg; ++ch)
        for (int m = 0; m < p.Mg; ++m)
          for (int t = 0; t < taps; ++t)
            c->wf[((size_t)(gi * p.Mg + m) * p.Cg + ch) * taps + (taps - 1 - t)] =
                w->c.f[((size_t)(gi * p.Cg + ch) * p.Mg + m) * taps + t];
    c->bias.assign(p.M, 0.f);
    if (b) {
      if (!b->is_const || b->c.numel() != p.M) return fail(who + ": bias must be constant [M]");
      c->bias = b->c.f;
      c->has_bias = true;
    }
    return true;
  }

  // ConvTranspose.  Stride 1: the Conv above on the convolution planner, f32
  // operands in every session.  Otherwise the phase decomposition
  // (vso_kernels.h, DeconvParams): k_deconv_tile for group 1, dilation 1, at
  // least kDeconvMinC channels on both sides and at most kDeconvMaxTaps taps
  // per phase and axis; k_deconv_direct for the rest, and for a stride-1 node
  // whose pads exceed d (k - 1) (the Conv's would be negative).
  static constexpr int kDeconvMinC = 16;
  static constexpr long kDeconvPairMinWgs = 1024;
  bool plan_conv_transpose(size_t ni, const Node& nd, Ins& in) {
    const std::string& in0 = nd.in[0];
    ConvPlan c;
    int sh = 1, sw = 1;
    if (!deconv_geometry(nd, in, &c, &sh, &sw) || !conv_absorb(ni, &c)) return false;
    flush_input(in0);
    flush_norm(in0);
    ConvParams& cp = c.p;
    cp.ep.bias = c.has_bias ? upload_vec(c.bias) : nullptr;
    if (c.has_bias && !cp.ep.bias) return false;
    cp.x = dptr(*in[0]);
    if (sh == 1 && sw == 1 && cp.pt >= 0 && cp.pl >= 0) {
      cp.w = upload_vec(c.wf);
      if (!cp.w || !(cp.y = make_out(c.out, c.oshape))) return false;
      return plan_conv_dense(in0, c, PREC_F32);
    }
    DeconvParams p{};
    p.x = cp.x;
    p.N = cp.N; p.C = cp.C; p.H = cp.H; p.W = cp.W; p.M = cp.M; p.Ho = cp.Ho; p.Wo = cp.Wo;
    p.G = cp.G; p.Cg = cp.Cg; p.Mg = cp.Mg;
    p.kh = cp.kh; p.kw = cp.kw; p.sh = sh; p.sw = sw; p.dh = cp.dh; p.dw = cp.dw;
    p.pt = cp.dh * (cp.kh - 1) - cp.pt;  // the node's own pads again
    p.pl = cp.dw * (cp.kw - 1) - cp.pl;
    p.ep = cp.ep;
    // the phase grid: q = (o + pad) div stride over the outputs of every phase
    p.qy0 = p.pt / sh; p.Qh = (p.Ho - 1 + p.pt) / sh - p.qy0 + 1;
    p.qx0 = p.pl / sw; p.Qw = (p.Wo - 1 + p.pl) / sw - p.qx0 + 1;
    const int taps = p.kh * p.kw;
    // c.wf (flipped, [M][Cg]) -> the node's W[c][mg][ky][kx], whatever conv_absorb folded in
    auto w_at = [&](int ch, int m, int ky, int kx) {
      const int gi = ch / p.Cg;
      return c.wf[((size_t)(gi * p.Mg + m) * p.Cg + (ch - gi * p.Cg)) * taps + (taps - 1 - (ky * p.kw + kx))];
    };
    p.tmy = (p.kh + sh - 1) / sh;
    p.tmx = (p.kw + sw - 1) / sw;
    const long mblocks = (p.M + kDeconvBM - 1) / kDeconvBM;
    const bool tile = deconv_tile_enabled() && p.G == 1 && p.dh == 1 && p.dw == 1 && p.C >= kDeconvMinC &&
                      p.M >= kDeconvMinC && p.tmy <= kDeconvMaxTaps && p.tmx <= kDeconvMaxTaps &&
                      (long)sh * sw * mblocks < 65536 && p.N < 65536;
    const char* name;
    void (*launch)(const DeconvParams&, hipStream_t);
    if (tile) {
      p.Mp = (int)mblocks * kDeconvBM;
      p.Cp = (p.C + 15) / 16 * 16;
      p.tiles_x = (p.Qw + 15) / 16;
      p.tiles = p.tiles_x * ((p.Qh + kDeconvTH - 1) / kDeconvTH);
      p.pitch = 16 + p.tmx - 1;
      // channels 4 apart in banks 16 apart: the MFMA B reads of lanes (r, g) are conflict free
      const int rows = (kDeconvTH + p.tmy - 1) * p.pitch;
      p.plane = rows + ((4 - rows) % 8 + 8) % 8;
      std::vector<float> wp((size_t)sh * sw * p.tmy * p.tmx * p.Mp * p.Cp, 0.f);
      for (int py = 0; py < sh; ++py)
        for (int px = 0; px < sw; ++px)
          for (int jy = 0; py + jy * sh < p.kh; ++jy)
            for (int jx = 0; px + jx * sw < p.kw; ++jx) {
              float* dst = wp.data() + (size_t)(((py * sw + px) * p.tmy + jy) * p.tmx + jx) * p.Mp * p.Cp;
              for (int m = 0; m < p.M; ++m)
                for (int ch = 0; ch < p.C; ++ch) dst[(size_t)m * p.Cp + ch] = w_at(ch, m, py + jy * sh, px + jx * sw);
            }
      p.w = static_cast<const float*>(upload_bytes(wp.data(), wp.size() * 4, "conv weight upload failed"));
      // both x phases per workgroup halve the workgroups: 10 % faster with 10064 of them (32 -> 16 k2 s2 at
      // 144x256, batch 8), the same at 1258 and 2736, 14 % slower at 342 (64 -> 32 k4 s2 at 72x128, batch 1:
      // 1.3 per CU) — profiles/NOTES.md, "ConvTranspose"
      const long pair_wgs = (long)p.N * p.tiles * sh * mblocks;
      p.sx = sw == 2 && (deconv_pair() < 0 ? pair_wgs >= kDeconvPairMinWgs : deconv_pair() != 0) ? 2 : 1;
      name = deconv_tile_name(p);
      launch = launch_deconv_tile;
    } else {
      std::vector<float> wd((size_t)p.C * p.Mg * taps);
      for (int ch = 0; ch < p.C; ++ch)
        for (int m = 0; m < p.Mg; ++m)
          for (int ky = 0; ky < p.kh; ++ky)
            for (int kx = 0; kx < p.kw; ++kx) wd[((size_t)ch * p.Mg + m) * taps + ky * p.kw + kx] = w_at(ch, m, ky, kx);
      p.w = upload_vec(wd);
      // per phase, its taps: k with (k d) mod s == phase, reading q - (k d) div s
      std::vector<int> tab;
      auto axis = [&](int kk, int ss, int dd) {
        const size_t start = tab.size();
        tab.resize(start + ss + 1 + 2 * (size_t)kk);
        size_t at = start + ss + 1, n = 0;
        for (int ph = 0; ph < ss; ++ph) {
          tab[start + ph] = (int)n;
          for (int q = 0; q < kk; ++q)
            if ((q * dd) % ss == ph) {
              tab[at + 2 * n] = q;
              tab[at + 2 * n + 1] = (q * dd) / ss;
              ++n;
            }
        }
        tab[start + ss] = (int)n;
      };
      axis(p.kh, sh, p.dh);
      p.o_yt = sh + 1;
      p.o_xs = (int)tab.size();
      axis(p.kw, sw, p.dw);
      p.o_xt = p.o_xs + sw + 1;
      p.taps = static_cast<const int*>(upload_bytes(tab.data(), tab.size() * sizeof(int)));
      if (!p.taps) return false;
      name = "vso::k_deconv_direct(vso::DeconvParams)";
      launch = launch_deconv_direct;
    }
    if (!p.w || !(p.y = make_out(c.out, c.oshape))) return false;
    auto pp = emit(name, p, launch);
    retarget_on_concat(c.out, pp, p.M);
    return true;
  }

  // ---- the other operators: one plan_<op> each -----------------------------
  static void fill_strides(const std::vector<int64_t>& shape, std::vector<int64_t>* st) {
    st->assign(shape.size(), 1);
    for (int k = (int)shape.size() - 2; k >= 0; --k) (*st)[k] = (*st)[k + 1] * shape[k + 1];
  }
  static int64_t inner_from(const std::vector<int64_t>& shape, size_t d0) {  // the product of dims d0 on
    int64_t n = 1;
    for (size_t d = d0; d < shape.size(); ++d) n *= shape[d];
    return n;
  }
  static std::vector<int64_t> ints(const Value& v) {
    return v.c.is_int ? v.c.i : std::vector<int64_t>(v.c.f.begin(), v.c.f.end());
  }

  bool plan_view(size_t, const Node& nd, Ins& in) {  // Reshape, Flatten, Squeeze, Unsqueeze: an alias
    std::vector<int64_t> shp;
    if (!infer_view(nd, operands(in), &shp, &err)) return false;
    if (index_vals.count(nd.in[0])) index_vals.insert(nd.out[0]);
    return set_runtime(nd.out[0], shp, in[0]->buf);
  }

  bool plan_alias(size_t, const Node& nd, Ins& in) {  // Identity, Dropout
    if (index_vals.count(nd.in[0])) index_vals.insert(nd.out[0]);
    return set_runtime(nd.out[0], in[0]->shape, in[0]->buf);
  }

  bool plan_unary(const Node& nd, Value& x, int act, float a0, float a1, const std::string* out = nullptr) {
    const std::string& o = out ? *out : nd.out[0];
    UnaryParams p{};
    p.x = dptr(x);
    p.act = act; p.a0 = a0; p.a1 = a1;
    if (!(p.y = make_out(o, x.shape))) return false;
    p.n = vals[o].numel();
    emit("vso::k_unary(vso::UnaryParams)", p, launch_unary);
    return true;
  }

  bool plan_cast(size_t ni, const Node& nd, Ins& in) {
    const int64_t to = nd.ai("to", DT_FLOAT);
    if (in[0]->qtype == DT_INT32) {  // a ConvInteger / MatMulInteger output: one conversion per element
      if (to != DT_FLOAT) return fail("Cast '" + nd.name + "': unsupported: an int32 tensor is cast to FLOAT only");
      const int* xp = reinterpret_cast<const int*>(s->bufs[in[0]->buf]);
      const long n = (long)in[0]->numel();
      const std::vector<int64_t> shape = in[0]->shape;
      float* y = make_out(nd.out[0], shape);
      if (!y) return false;
      emit("vso::k_cast_i32(vso::CastI32Params)", CastI32Params{xp, y, n}, launch_cast_i32);
      return true;
    }
    // float16 storage semantics: round to the nearest half (the values stay
    // f32 in HBM; later ops compute in f32, a superset of the f16 precision)
    if (to == DT_FLOAT16) return plan_unary(nd, *in[0], ACT_F16, 0.f, 0.f);
    // an index tensor holds exact integers in f32: its integer types are the same bytes
    const bool index = index_vals.count(nd.in[0]) && (to == DT_INT64 || to == DT_INT32 || to == DT_UINT8);
    if (to != DT_FLOAT && !index) return fail("Cast of a runtime tensor to a non-float type");
    return plan_alias(ni, nd, in);
  }

  bool plan_activation(size_t ni, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    if (nd.op == "PRelu") {
      // unidirectional: the slope broadcasts to x, never x to the slope
      const std::vector<int64_t>& ss = in[1]->shape;
      bool uni = ss.size() <= xs.size();
      for (size_t d = 0; uni && d < ss.size(); ++d)
        uni = ss[d] == 1 || ss[d] == xs[d + xs.size() - ss.size()];
      if (!uni) return fail("PRelu '" + nd.name + "': slope does not broadcast to the input");
      return plan_binary(nd, in[0], in[1], BIN_PRELU);
    }
    Epilogue ep{};
    if (!act_of(nd, &ep, 0)) return fail(nd.op + " '" + nd.name + "': non-constant parameters");
    const auto hw = hswish.find(ni);
    if (hw != hswish.end() && !done.count(hw->second)) {  // with its Mul: x * HardSigmoid(x), written as the Mul's output
      done.insert(hw->second);
      return plan_unary(nd, *in[0], ACT_HSWISH, ep.a0, ep.a1, &g.nodes[hw->second].out[0]);
    }
    return plan_unary(nd, *in[0], ep.act, ep.a0, ep.a1);
  }

  bool plan_arith(size_t ni, const Node& nd, Ins& in) {
    const std::string& op = nd.op;
    const auto gf = gelu.find(ni);
    if (gf != gelu.end()) {  // the head of an erf GELU no producer absorbed: one launch, written as the pattern's output
      Value* xv = val(gf->second.x);
      if (!xv || xv->is_const) return fail("Erf GELU of a constant (node '" + nd.name + "')");
      return plan_unary(nd, *xv, ACT_GELU, 0.f, 0.f, &g.nodes[gf->second.last].out[0]);
    }
    return plan_binary(nd, in[0], in[1], op == "Add" ? BIN_ADD : op == "Sub" ? BIN_SUB : op == "Mul" ? BIN_MUL : BIN_DIV);
  }

  bool plan_binary(const Node& nd, Value* a, Value* b, int op) {
    const size_t ra = a->shape.size(), rb = b->shape.size(), rk = std::max(ra, rb);
    if (rk > (size_t)kMaxDims) return fail(nd.op + ": rank > 6");
    std::vector<int64_t> os(rk);
    for (size_t d = 0; d < rk; ++d) {
      const int64_t da = d + ra >= rk ? a->shape[d + ra - rk] : 1, db = d + rb >= rk ? b->shape[d + rb - rk] : 1;
      if (da != db && da != 1 && db != 1) return fail(nd.op + " '" + nd.name + "': shapes do not broadcast");
      os[d] = std::max(da, db);
    }
    std::vector<int64_t> sta, stb;
    fill_strides(a->shape, &sta);
    fill_strides(b->shape, &stb);
    BinParams p{};
    p.nd = (int)rk;
    for (size_t d = 0; d < rk; ++d) {
      p.dims[d] = (int)os[d];
      const int64_t da = d + ra >= rk ? a->shape[d + ra - rk] : 1, db = d + rb >= rk ? b->shape[d + rb - rk] : 1;
      p.sa[d] = da == 1 ? 0 : sta[d + ra - rk];
      p.sb[d] = db == 1 ? 0 : stb[d + rb - rk];
    }
    p.op = op;
    p.a = operand(*a);
    p.b = operand(*b);
    if (!p.a || !p.b) return false;
    if (!(p.y = make_out(nd.out[0], os))) return false;
    p.n = vals[nd.out[0]].numel();
    emit(binary_kernel_name(p), p, launch_binary);
    return true;
  }

  // One strided copy (k_copy; k_copy_rows where it is rows of one contiguous
  // run): iteration space `iter`, written at dst_off, read from src_start by
  // src_step through src_perm, `fill` outside the source
  bool plan_copy_into(const float* src, const std::vector<int64_t>& src_shape, float* dst,
                      const std::vector<int64_t>& dst_shape, const std::vector<int64_t>& iter, const std::vector<int64_t>& dst_off,
                      const std::vector<int64_t>& src_start, const std::vector<int64_t>& src_step,
                      const std::vector<int64_t>& src_perm, float fill) {
    const size_t rk = iter.size();
    if (rk > (size_t)kMaxDims) return fail("copy: rank > 6");
    std::vector<int64_t> sst, dst_st;
    fill_strides(src_shape, &sst);
    fill_strides(dst_shape, &dst_st);
    CopyParams p{};
    p.nd = (int)rk;
    p.n = 1;
    long base = 0;
    for (size_t d = 0; d < rk; ++d) {
      p.size[d] = (int)iter[d];
      p.n *= iter[d];
      p.dst_stride[d] = dst_st[d];
      base += dst_off[d] * dst_st[d];
      const int64_t sd = src_perm.empty() ? (int64_t)d : src_perm[d];
      p.src_stride[d] = sst[sd];
      p.start[d] = (int)src_start[d];
      p.step[d] = (int)src_step[d];
      p.lim[d] = (int)src_shape[sd];
    }
    p.dst_base = base;
    p.src_base = 0;
    p.src = src;
    p.dst = dst;
    p.fill = fill;
    if (p.n == 0) return true;
    // a block copy (Concat / Split / Slice of whole trailing dims, no fill):
    // rows of one contiguous run in both tensors -> k_copy_rows (16-byte moves)
    bool block = src_perm.empty();
    for (size_t d = 0; block && d < rk; ++d)
      block = src_step[d] == 1 && src_start[d] >= 0 && src_start[d] + iter[d] <= src_shape[d];
    if (block) {
      int d = (int)rk - 1;
      int64_t inner = 1;
      while (d >= 0 && iter[d] == src_shape[d] && iter[d] == dst_shape[d]) inner *= iter[d--];
      if (d >= 0) inner *= iter[d--];
      bool one_outer = true;  // at most one outer dimension left (dim 0)
      for (int k = 0; k <= d && k < (int)rk; ++k)
        if (k > 0 && iter[k] != 1) one_outer = false;
      if (one_outer && d <= 0) {
        RowCopyParams q{};
        q.src = src;
        q.dst = dst;
        q.inner = inner;
        q.rows = d == 0 ? iter[0] : 1;
        q.src_row = d == 0 ? sst[0] : 0;
        q.dst_row = d == 0 ? dst_st[0] : 0;
        int64_t sb = 0;
        for (size_t k = 0; k < rk; ++k) sb += src_start[k] * sst[k];
        q.src_base = sb;
        q.dst_base = base;
        emit(row_copy_name(q), q, launch_copy_rows);
        return true;
      }
    }
    emit("vso::k_copy(vso::CopyParams)", p, launch_copy);
    return true;
  }
  // ... a whole tensor `x` (shape xs) into `name` (shape os), from `start` by `step`
  bool plan_copy_out(const std::string& name, const std::vector<int64_t>& os, const float* x,
                     const std::vector<int64_t>& xs, const std::vector<int64_t>& start,
                     const std::vector<int64_t>& step, const std::vector<int64_t>& perm, float fill) {
    float* y = make_out(name, os);
    return y && plan_copy_into(x, xs, y, os, os, std::vector<int64_t>(os.size(), 0), start, step, perm, fill);
  }

  bool plan_pool(size_t, const Node& nd, Ins& in) {  // MaxPool, AveragePool
    const std::string& op = nd.op;
    const std::vector<int64_t>& xs = in[0]->shape;
    if (xs.size() != 4) return fail(op + ": 2D only");
    std::vector<int64_t> k = nd.ais("kernel_shape"), st = nd.ais("strides"), dl = nd.ais("dilations"), pd = nd.ais("pads");
    if (k.size() != 2) return fail(op + ": kernel_shape must be 2D");
    if (!pd.empty() && pd.size() != 4) return fail(op + ": pads must have 4 values");
    if (nd.ai("storage_order", 0) != 0) return fail(op + ": storage_order 1 is not supported");
    if (nd.out.size() > 1 && !nd.out[1].empty()) return fail(op + ": the Indices output is not supported");
    PoolParams p{};
    p.N = (int)xs[0]; p.C = (int)xs[1]; p.H = (int)xs[2]; p.W = (int)xs[3];
    p.kh = (int)k[0]; p.kw = (int)k[1];
    p.sh = st.size() > 0 ? (int)st[0] : 1; p.sw = st.size() > 1 ? (int)st[1] : 1;
    p.dh = dl.size() > 0 ? (int)dl[0] : 1; p.dw = dl.size() > 1 ? (int)dl[1] : 1;
    int pads[4] = {0, 0, 0, 0};  // top, left, bottom, right
    for (size_t q = 0; q < pd.size(); ++q) pads[q] = (int)pd[q];
    same_pads(nd.as("auto_pad", "NOTSET"), p, pads);
    p.pt = pads[0]; p.pl = pads[1];
    p.He = p.H + pads[2]; p.We = p.W + pads[3];
    const bool ceil_mode = nd.ai("ceil_mode", 0) != 0;
    auto osz = [&](int i, int p0, int p1, int kk, int ss, int dd) {
      const int num = i + p0 + p1 - dd * (kk - 1) - 1;
      int o = (ceil_mode ? (num + ss - 1) / ss : num / ss) + 1;
      if (ceil_mode && (o - 1) * ss >= i + p0) --o;
      return o;
    };
    p.Ho = osz(p.H, pads[0], pads[2], p.kh, p.sh, p.dh);
    p.Wo = osz(p.W, pads[1], pads[3], p.kw, p.sw, p.dw);
    p.max_mode = op == "MaxPool";
    p.count_include_pad = (int)nd.ai("count_include_pad", 0);
    p.x = dptr(*in[0]);
    if (!(p.y = make_out(nd.out[0], {xs[0], xs[1], p.Ho, p.Wo}))) return false;
    emit("vso::k_pool(vso::PoolParams)", p, launch_pool);
    return true;
  }

  bool plan_global_pool(size_t, const Node& nd, Ins& in) {  // GlobalAveragePool
    const std::vector<int64_t>& xs = in[0]->shape;
    RowParams p{};
    p.x = dptr(*in[0]);
    p.rows = xs[0] * xs[1];
    p.inner = inner_from(xs, 2);
    std::vector<int64_t> os = {xs[0], xs[1]};
    for (size_t d = 2; d < xs.size(); ++d) os.push_back(1);
    if (!(p.y = make_out(nd.out[0], os))) return false;
    emit(gap_kernel_name(p), p, launch_gap);
    return true;
  }

  // ReduceMean over exactly H and W of a rank-4 tensor: GlobalAveragePool's
  // kernels; keepdims 0 is the same buffer seen as [N, C].  Over the last axis
  // it may head a decomposed LayerNorm (find_layernorm): one k_layer_norm
  // launch; outside that pattern it is refused as any other axis set.
  bool plan_reduce_mean(size_t ni, const Node& nd, Ins& in) {
    const std::string who = "ReduceMean '" + nd.name + "'";
    const std::vector<int64_t>& xs = in[0]->shape;
    LnMatch lm;
    if (xs.size() >= 2 && !in[0]->is_const && find_layernorm(ni, xs, &lm)) {
      for (size_t q : lm.nodes) done.insert(q);
      return emit_layer_norm(*in[0], xs.back(), lm.has_gamma ? &lm.gamma : nullptr, lm.has_beta ? &lm.beta : nullptr,
                             lm.eps, lm.out);
    }
    if (xs.size() != 4) return fail(who + ": rank-4 input only");
    std::vector<int64_t> axes = nd.ais("axes");
    if (in.size() > 1 && in[1]) {  // opset 18 on: an input
      if (!in[1]->is_const) return fail(who + ": constant axes only");
      axes = ints(*in[1]);
    }
    if (axes.empty() && nd.ai("noop_with_empty_axes", 0) != 0) return plan_alias(ni, nd, in);
    return plan_reduce_mean_hw(ni, nd, in, axes);
  }

  // ---- LayerNormalization --------------------------------------------------
  // one k_layer_norm launch: x's rows of D contiguous elements -> `out`
  bool emit_layer_norm(Value& x, int64_t D, const Const* scale, const Const* shift, float eps, const std::string& out) {
    LayerNormParams p{};
    p.x = dptr(x);
    p.D = (int)D;
    p.rows = D > 0 ? x.numel() / D : 0;
    p.eps = eps;
    if (scale && !(p.scale = upload_vec(scale->f))) return false;
    if (shift && !(p.shift = upload_vec(shift->f))) return false;
    if (!(p.y = make_out(out, x.shape))) return false;
    emit(layer_norm_name(p), p, launch_layer_norm);
    return true;
  }

  bool plan_layer_norm(size_t, const Node& nd, Ins& in) {
    const std::string who = "LayerNormalization '" + nd.name + "'";
    Value* x = in[0];
    const int64_t rk = (int64_t)x->shape.size();
    if (rk < 2) return fail(who + ": rank >= 2 only");
    int64_t ax = nd.ai("axis", -1);
    if (ax < 0) ax += rk;
    if (ax < 0 || ax >= rk) return fail(who + ": axis out of range");
    if (nd.ai("stash_type", 1) != 1) return fail(who + ": stash_type 1 only");
    for (size_t k = 1; k < nd.out.size(); ++k) {
      bool used = !nd.out[k].empty() && consumers[nd.out[k]] > 0;
      for (const IO& o : g.outputs) used = used || (!nd.out[k].empty() && o.name == nd.out[k]);
      if (used) return fail(who + ": the Mean / InvStdDev outputs are not supported");
    }
    const int64_t D = inner_from(x->shape, (size_t)ax);
    Value* sc = in.size() > 1 ? in[1] : nullptr;
    Value* sh = in.size() > 2 ? in[2] : nullptr;
    if (!sc || !sc->is_const || (sh && !sh->is_const)) return fail(who + ": constant Scale and B only");
    if (sc->c.numel() != D || (sh && sh->c.numel() != D)) return fail(who + ": Scale / B must have the normalised extent's elements");
    if (D >= (1LL << 31)) return fail(who + ": rows of 2^31 elements or more");
    return emit_layer_norm(*x, D, &sc->c, sh ? &sh->c : nullptr, nd.af("epsilon", 1e-5f), nd.out[0]);
  }

  // LayerNorm as PyTorch exports it below opset 17, from its first ReduceMean `ni`:
  //   m = ReduceMean(x, axes [-1], keepdims 1); d = Sub(x, m); Pow(d, 2) | Mul(d, d);
  //   ReduceMean(axes [-1], keepdims 1); Add(eps); Sqrt; Div(d, .) [; Mul(gamma)] [; Add(beta)]
  // every interior value read inside the pattern only (d by its square and the
  // Div), eps a scalar, gamma / beta constants of 1 or D elements.
  struct LnMatch {
    std::vector<size_t> nodes;  // behind `ni`
    float eps;
    Const gamma, beta;
    bool has_gamma = false, has_beta = false;
    std::string out;
  };
  bool last_axis_mean(const Node& nd, int64_t rk) {
    if (nd.op != "ReduceMean" || nd.in.empty() || nd.ai("keepdims", 1) != 1) return false;
    std::vector<int64_t> axes = nd.ais("axes");
    Const t;
    if (nd.in.size() > 1 && !nd.in[1].empty()) {
      const Const* c = const_of(nd.in[1], &t);
      if (!c) return false;
      axes = ints_of(*c);
    }
    return axes.size() == 1 && (axes[0] == -1 || axes[0] == rk - 1);
  }
  static std::vector<int64_t> ints_of(const Const& c) {
    return c.is_int ? c.i : std::vector<int64_t>(c.f.begin(), c.f.end());
  }
  bool find_layernorm(size_t ni, const std::vector<int64_t>& xs, LnMatch* m) {
    const Node& rm = g.nodes[ni];
    const int64_t rk = (int64_t)xs.size(), D = xs.back();
    if (!last_axis_mean(rm, rk)) return false;
    const std::string& x = rm.in[0];
    const int sb = sole_consumer(rm.out[0], ni);
    if (sb < 0 || g.nodes[sb].op != "Sub" || g.nodes[sb].in.size() != 2 || g.nodes[sb].in[0] != x ||
        g.nodes[sb].in[1] != rm.out[0])
      return false;
    const std::string& d = g.nodes[sb].out[0];
    for (const IO& o : g.outputs)
      if (o.name == d) return false;
    // d's readers: its square and the Div, nothing else
    int sq = -1, dv = -1, reads = 0;
    for (size_t k = (size_t)sb + 1; k < g.nodes.size(); ++k)
      for (const std::string& i : g.nodes[k].in)
        if (i == d) {
          ++reads;
          const Node& c = g.nodes[k];
          double e;
          if (c.op == "Pow" && c.in.size() == 2 && c.in[0] == d && scalar_of(c.in[1], &e) && e == 2.0) sq = (int)k;
          else if (c.op == "Mul" && c.in.size() == 2 && c.in[0] == d && c.in[1] == d) sq = (int)k;
          else if (c.op == "Div" && c.in.size() == 2 && c.in[0] == d && c.in[1] != d) dv = (int)k;
          else return false;
        }
    if (sq < 0 || dv < 0 || reads != (g.nodes[sq].op == "Mul" ? 3 : 2) || consumers[d] != reads) return false;
    const int r2 = sole_consumer(g.nodes[sq].out[0], (size_t)sq);
    if (r2 < 0 || !last_axis_mean(g.nodes[r2], rk)) return false;
    const int ae = sole_consumer(g.nodes[r2].out[0], (size_t)r2);
    double eps;
    if (ae < 0 || g.nodes[ae].op != "Add" || !with_scalar(g.nodes[ae], g.nodes[r2].out[0], &eps)) return false;
    const int sr = sole_consumer(g.nodes[ae].out[0], (size_t)ae);
    if (sr < 0 || g.nodes[sr].op != "Sqrt") return false;
    if (sole_consumer(g.nodes[sr].out[0], (size_t)sr) != dv || g.nodes[dv].in[1] != g.nodes[sr].out[0]) return false;
    m->eps = (float)eps;
    m->nodes = {(size_t)sb, (size_t)sq, (size_t)r2, (size_t)ae, (size_t)sr, (size_t)dv};
    m->out = g.nodes[dv].out[0];
    size_t last = (size_t)dv;
    auto affine = [&](const char* op, Const* into) {
      const int k = sole_consumer(m->out, last);
      if (k < 0 || g.nodes[k].op != op || g.nodes[k].in.size() != 2) return false;
      const Node& nd = g.nodes[k];
      Const t;
      const Const* c = const_of(nd.in[0] == m->out ? nd.in[1] : nd.in[0], &t);
      if (!c || c->is_int || (c->numel() != 1 && !(c->numel() == D && c->dims.back() == D))) return false;
      *into = *c;
      if (c->numel() == 1) into->f.assign((size_t)D, c->f[0]);
      m->nodes.push_back((size_t)k);
      m->out = nd.out[0];
      last = (size_t)k;
      return true;
    };
    m->has_gamma = affine("Mul", &m->gamma);
    m->has_beta = affine("Add", &m->beta);
    for (size_t q : m->nodes)
      if (done.count(q)) return false;
    return true;
  }

  // ReduceMean over exactly H and W: see plan_reduce_mean
  bool plan_reduce_mean_hw(size_t, const Node& nd, Ins& in, std::vector<int64_t> axes) {
    const std::string who = "ReduceMean '" + nd.name + "'";
    const std::vector<int64_t>& xs = in[0]->shape;
    for (int64_t& a : axes) a = a < 0 ? a + 4 : a;
    std::sort(axes.begin(), axes.end());
    if (axes != std::vector<int64_t>{2, 3}) return fail(who + ": the two spatial axes of an NCHW tensor only");
    RowParams p{};
    p.x = dptr(*in[0]);
    p.rows = xs[0] * xs[1];
    p.inner = xs[2] * xs[3];
    const bool keep = nd.ai("keepdims", 1) != 0;
    if (!(p.y = make_out(nd.out[0], keep ? std::vector<int64_t>{xs[0], xs[1], 1, 1} : std::vector<int64_t>{xs[0], xs[1]})))
      return false;
    emit(gap_kernel_name(p), p, launch_gap);
    return true;
  }

  bool plan_instance_norm(size_t, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    if (!in[1]->is_const || !in[2]->is_const) return fail("InstanceNormalization: constant scale/B only");
    if (xs.size() < 3) return fail("InstanceNormalization: rank >= 3 only");
    float* y = make_out(nd.out[0], xs);
    return y && plan_norm(dptr(*in[0]), y, (int)xs[0], (int)xs[1], 0, (int)xs[1], inner_from(xs, 2), nd, in[1], in[2],
                          ACT_NONE);
  }

  // InstanceNormalization (node `nd`, constant scale / B) of planes c0 .. c0+C-1
  // of an [N][ctot][inner] tensor: k_norm_plane, or k_norm_stats + k_norm_apply
  bool plan_norm(const float* x, float* y, int N, int C, int c0, int ctot, int64_t inner, const Node& nd, Value* sc,
                 Value* sh, int act, const std::string* direct = nullptr, const std::string* defer = nullptr) {
    if (sc->c.numel() != C || sh->c.numel() != C) return fail("InstanceNormalization '" + nd.name + "': scale/B size");
    NormParams p{};
    p.x = x; p.y = y;
    p.N = N; p.C = C; p.c0 = c0; p.ctot = ctot;
    p.inner = inner;
    p.scale = upload(sc->c);
    p.shift = upload(sh->c);
    p.eps = nd.af("epsilon", 1e-5f);
    p.act = act;
    p.chunk = kNormChunk;
    p.chunks = (int)((inner + kNormChunk - 1) / kNormChunk);
    if (!p.scale || !p.shift || !dalloc(&p.stats, (size_t)N * C * std::max(p.chunks, 1) * 3 * 4)) return false;
    if (inner == 0 || N * C == 0) return true;
    std::shared_ptr<NormParams> pp;
    if (!defer && norm_plane_fits(inner) && norm_plane_enabled()) {
      pp = emit(norm_plane_name(inner), p, launch_norm_plane);
    } else {
      pp = emit("vso::k_norm_stats(vso::NormParams)", p, launch_norm_stats);
      if (defer) {  // the apply step runs in the consumer (k_conv_thin) or, failing that, flush_norm
        norm_pending[*defer] = pp;
        return true;
      }
      add("vso::k_norm_apply(vso::NormParams)", pp, launch_norm_apply);
    }
    if (direct)  // in place on the conv's output, wherever that now lies
      cat_patch[*direct].push_back([pp](float* base, int ctot) { pp->x = pp->y = base; pp->ctot = ctot; });
    return true;
  }

  bool plan_batch_norm(size_t, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    for (int k = 1; k <= 4; ++k)
      if (!in[k]->is_const) return fail("BatchNormalization: constant parameters only");
    const int C = (int)xs[1];
    std::vector<float> sc(C), sh(C);
    const BnConsts b = bn_consts(nd);
    for (int c = 0; c < C; ++c) {
      const double a = b.a(c);
      sc[c] = (float)a;
      sh[c] = (float)(b.B.f[c] - b.mean.f[c] * a);
    }
    AffineParams p{};
    p.x = dptr(*in[0]);
    p.C = C;
    p.inner = inner_from(xs, 2);
    p.scale = upload_vec(sc);
    p.shift = upload_vec(sh);
    if (!(p.y = make_out(nd.out[0], xs))) return false;
    p.n = vals[nd.out[0]].numel();
    emit("vso::k_affine(vso::AffineParams)", p, launch_affine);
    return true;
  }

  bool plan_softmax(size_t ni, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    // opset 13 on: along `axis` (default -1), here the last axis only.  Before:
    // the input flattened to 2-D at `axis` (default 1), each row normalised.
    const bool flat = g.opset > 0 && g.opset < 13;
    const int64_t rk = (int64_t)xs.size();
    int64_t ax = nd.ai("axis", flat ? 1 : -1);
    if (ax < 0) ax += rk;
    if (ax < 0 || ax >= rk) return fail("Softmax: axis out of range");
    if (!flat && ax != rk - 1) {
      if (rk == 4 && ax == 1) return plan_softmax_head(ni, nd, in, HEAD_SOFTMAX);
      return fail("Softmax: last axis only");
    }
    if (!flush_head(nd.in[0])) return false;
    RowParams p{};
    p.x = dptr(*in[0]);
    p.inner = inner_from(xs, (size_t)ax);
    p.rows = in[0]->numel() / std::max<int64_t>(p.inner, 1);
    if (!(p.y = make_out(nd.out[0], xs))) return false;
    emit("vso::k_softmax(vso::RowParams)", p, launch_softmax);
    return true;
  }

  // ---- class heads (vso_head.hip) ------------------------------------------
  static bool is_head_op(const std::string& op) {
    return op == "Softmax" || op == "LogSoftmax" || op == "ArgMax" || op == "ReduceMax";
  }
  // Resizes read by one class head only: plan_resize leaves them to it
  void find_heads() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& nd = g.nodes[k];
      if (nd.op != "Resize" || nd.out.empty()) continue;
      const int c = sole_consumer(nd.out[0], k);
      if (c >= 0 && is_head_op(g.nodes[c].op) && g.nodes[c].in[0] == nd.out[0]) head_up.insert(nd.out[0]);
    }
  }
  // a constant a later node of a pattern reads, when a Constant node after the
  // pattern's head produces it: folded now
  Value* const_ahead(const std::string& name) {
    if (name.empty()) return nullptr;
    if (!val(name)) {
      const int p = producer(name);
      if (p < 0 || g.nodes[p].op != "Constant" || done.count((size_t)p) || !plan_node((size_t)p)) return nullptr;
      done.insert((size_t)p);
    }
    Value* v = val(name);
    return v && v->is_const ? v : nullptr;
  }
  // the channel axis of a rank-4 tensor, as 1 or -3
  static bool channel_axis(const std::vector<int64_t>& xs, int64_t ax) { return xs.size() == 4 && (ax == 1 || ax == -3); }

  // One k_class_head launch over `in_name` ([N, C, H, W]; its pending Resize
  // computed on the fly): classes [c0, c0 + n) for the softmax forms -> `out`
  // of shape `os`.  `fused`: the launch stands for more than its own node.
  bool emit_head(const std::string& in_name, const std::string& who, int op, int64_t c0, int64_t n, int last, float k,
                 const std::string& out, const std::vector<int64_t>& os, bool fused) {
    Value& x = vals[in_name];
    const std::vector<int64_t> xs = x.shape;
    HeadParams p{};
    auto hp = head_pending.find(in_name);
    if (hp != head_pending.end()) {
      p.rz = hp->second;
      head_pending.erase(hp);
      fused = true;
    } else {
      p.rz.x = dptr(x);
      p.rz.N = (int)xs[0]; p.rz.C = (int)xs[1];
      p.rz.H = p.rz.Ho = (int)xs[2]; p.rz.W = p.rz.Wo = (int)xs[3];
      p.rz.sy = p.rz.sx = 1.f;
    }
    if (xs[1] < 1) return fail(who + ": no classes");
    if (x.numel() >= (1LL << 31) || (int64_t)p.rz.N * p.rz.C * p.rz.H * p.rz.W >= (1LL << 31))
      return fail(who + ": input of 2^31 elements or more");
    p.op = op; p.c0 = (int)c0; p.n = (int)n; p.last = last; p.k = k;
    if (!(p.y = make_out(out, os))) return false;
    emit(head_kernel_name(p), p, launch_head);
    if (fused && head_enabled()) s->head_nodes++;
    return true;
  }

  // Softmax / LogSoftmax over the channel axis.  A Slice (axis 1, step 1), a
  // Split with one used output or a Gather (axis 1, one constant index) that
  // alone reads the result makes it the selected-channels form.
  bool plan_softmax_head(size_t ni, const Node& nd, Ins& in, int op) {
    const std::vector<int64_t> xs = in[0]->shape;
    const int64_t C = xs[1];
    int64_t c0 = 0, n = C;
    std::string out = nd.out[0];
    std::vector<int64_t> os = xs;
    const int k = head_enabled() ? sole_consumer(nd.out[0], ni) : -1;
    if (k >= 0 && g.nodes[k].in[0] == nd.out[0]) {
      const Node& cn = g.nodes[k];
      bool take = false;
      int64_t b = 0, e = 0;
      if (cn.op == "Slice") {
        for (size_t q = 1; q < cn.in.size(); ++q) const_ahead(cn.in[q]);
        if (slice_range(cn, C, &b, &e) && e > b) { take = true; c0 = b; n = e - b; os[1] = n; out = cn.out[0]; }
      } else if (cn.op == "Split") {
        const Value* sp = cn.in.size() > 1 ? const_ahead(cn.in[1]) : nullptr;
        int used = -1, nused = 0;
        for (size_t q = 0; q < cn.out.size(); ++q) {
          bool u = !cn.out[q].empty() && consumers[cn.out[q]] > 0;
          for (const IO& o : g.outputs) u = u || (!cn.out[q].empty() && o.name == cn.out[q]);
          if (u) { used = (int)q; ++nused; }
        }
        int64_t ax = 0;
        std::vector<int64_t> sizes;
        if (nused == 1 && (cn.in.size() < 2 || cn.in[1].empty() || sp) && split_sizes(cn, xs, sp, &ax, &sizes) && ax == 1 &&
            sizes[used] > 0) {
          for (int q = 0; q < used; ++q) b += sizes[q];
          take = true; c0 = b; n = sizes[used]; os[1] = n; out = cn.out[used];
        }
        err.clear();  // (a Split this declined reports its own error when it is planned)
      } else if (cn.op == "Gather" && cn.in.size() > 1) {
        const Value* iv = const_ahead(cn.in[1]);
        int64_t ax = cn.ai("axis", 0);
        if (ax < 0) ax += 4;
        if (iv && ax == 1 && iv->c.numel() == 1 && iv->c.dims.size() <= 1) {
          int64_t idx = ints(*iv)[0];
          if (idx < 0) idx += C;
          if (idx >= 0 && idx < C) {
            take = true; c0 = idx; n = 1; out = cn.out[0];
            if (iv->c.dims.empty()) os = {xs[0], xs[2], xs[3]};
            else os[1] = 1;
          }
        }
      }
      if (take) done.insert((size_t)k);
    }
    return emit_head(nd.in[0], nd.op + " '" + nd.name + "'", op, c0, n, 0, 0.f, out, os, out != nd.out[0]);
  }

  bool plan_log_softmax(size_t ni, const Node& nd, Ins& in) {
    const bool flat = g.opset > 0 && g.opset < 13;
    if (flat || !channel_axis(in[0]->shape, nd.ai("axis", -1)))
      return fail("LogSoftmax '" + nd.name + "': the channel axis of rank-4 input only (opset 13 on)");
    return plan_softmax_head(ni, nd, in, HEAD_LOGSOFTMAX);
  }

  // ArgMax over the channel axis: the index as a float holding the exact
  // integer (an index tensor: plan_cast).  ArgMax -> Equal(constant scalar) ->
  // Cast(FLOAT), each read by the next only, is the ArgMax == k form — with
  // VSO_HEAD=0 too: Equal has no launch of its own.
  bool plan_argmax(size_t ni, const Node& nd, Ins& in) {
    const std::string who = "ArgMax '" + nd.name + "'";
    const std::vector<int64_t> xs = in[0]->shape;
    if (!channel_axis(xs, nd.ai("axis", 0))) return fail(who + ": the channel axis of rank-4 input only");
    if (xs[1] >= (1 << 24)) return fail(who + ": 2^24 classes or more");
    const int64_t keep = nd.ai("keepdims", 1), last = nd.ai("select_last_index", 0);
    if ((keep != 0 && keep != 1) || (last != 0 && last != 1)) return fail(who + ": keepdims / select_last_index must be 0 or 1");
    const std::vector<int64_t> os = keep ? std::vector<int64_t>{xs[0], 1, xs[2], xs[3]} : std::vector<int64_t>{xs[0], xs[2], xs[3]};
    const int k1 = sole_consumer(nd.out[0], ni);
    if (k1 >= 0 && g.nodes[k1].op == "Equal" && g.nodes[k1].in.size() == 2) {
      const Node& eq = g.nodes[k1];
      const Value* cv = const_ahead(eq.in[0] == nd.out[0] ? eq.in[1] : eq.in[0]);
      const int k2 = sole_consumer(eq.out[0], (size_t)k1);
      if (cv && cv->c.numel() == 1 && k2 >= 0 && g.nodes[k2].op == "Cast" && g.nodes[k2].ai("to", DT_FLOAT) == DT_FLOAT) {
        done.insert((size_t)k1);
        done.insert((size_t)k2);
        const float kv = cv->c.is_int ? (float)cv->c.i[0] : cv->c.f[0];
        return emit_head(nd.in[0], who, HEAD_ARGMAX_EQ, 0, 1, (int)last, kv, g.nodes[k2].out[0], os, true);
      }
    }
    if (!emit_head(nd.in[0], who, HEAD_ARGMAX, 0, 1, (int)last, 0.f, nd.out[0], os, false)) return false;
    index_vals.insert(nd.out[0]);
    return true;
  }

  // ReduceMax over the channel axis alone
  bool plan_reduce_max(size_t, const Node& nd, Ins& in) {
    const std::string who = "ReduceMax '" + nd.name + "'";
    const std::vector<int64_t> xs = in[0]->shape;
    std::vector<int64_t> axes = nd.ais("axes");
    if (in.size() > 1 && in[1]) {  // opset 18 on: an input
      if (!in[1]->is_const) return fail(who + ": constant axes only");
      axes = ints(*in[1]);
    }
    if (axes.size() != 1 || !channel_axis(xs, axes[0])) return fail(who + ": over the channel axis of rank-4 input only");
    const int64_t keep = nd.ai("keepdims", 1);
    if (keep != 0 && keep != 1) return fail(who + ": keepdims must be 0 or 1");
    const std::vector<int64_t> os = keep ? std::vector<int64_t>{xs[0], 1, xs[2], xs[3]} : std::vector<int64_t>{xs[0], xs[2], xs[3]};
    return emit_head(nd.in[0], who, HEAD_MAX, 0, 1, 0, 0.f, nd.out[0], os, false);
  }

  // Gather of a runtime tensor by one constant index: a strided copy, the axis
  // dropped for a scalar index
  bool plan_gather(size_t, const Node& nd, Ins& in) {
    const std::string who = "Gather '" + nd.name + "'";
    const std::vector<int64_t>& xs = in[0]->shape;
    const size_t rk = xs.size();
    if (in.size() < 2 || !in[1] || !in[1]->is_const) return fail(who + ": constant indices only");
    if (in[0]->is_const) return fail(who + ": constant data with a runtime index");
    if (in[1]->c.numel() != 1 || in[1]->c.dims.size() > 1) return fail(who + ": a scalar or one-element index only");
    int64_t ax = nd.ai("axis", 0);
    if (ax < 0) ax += (int64_t)rk;
    if (ax < 0 || ax >= (int64_t)rk) return fail(who + ": axis out of range");
    int64_t idx = ints(*in[1])[0];
    if (idx < 0) idx += xs[ax];
    if (idx < 0 || idx >= xs[ax]) return fail(who + ": index out of range");
    std::vector<int64_t> os = xs, start(rk, 0);
    os[ax] = 1;
    start[ax] = idx;
    if (index_vals.count(nd.in[0])) index_vals.insert(nd.out[0]);
    if (!plan_copy_out(nd.out[0], os, dptr(*in[0]), xs, start, std::vector<int64_t>(rk, 1), {}, 0.f)) return false;
    if (in[1]->c.dims.empty()) vals[nd.out[0]].shape.erase(vals[nd.out[0]].shape.begin() + ax);
    return true;
  }

  bool plan_transpose(size_t, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    std::vector<int64_t> perm = nd.ais("perm");
    const size_t rk = xs.size();
    if (perm.empty()) for (size_t k = 0; k < rk; ++k) perm.push_back((int64_t)(rk - 1 - k));
    std::vector<int64_t> os(rk);
    for (size_t k = 0; k < rk; ++k) os[k] = xs[perm[k]];
    return plan_copy_out(nd.out[0], os, dptr(*in[0]), xs, std::vector<int64_t>(rk, 0), std::vector<int64_t>(rk, 1),
                         perm, 0.f);
  }

  bool plan_pad(size_t, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    const std::string mode = nd.as("mode", "constant");
    if (mode != "constant") return fail("Pad: constant mode only");
    std::vector<int64_t> pads = nd.ais("pads");
    if (in.size() > 1 && in[1]) {
      if (!in[1]->is_const) return fail("Pad: constant pads only");
      pads = ints(*in[1]);
    }
    float value = nd.af("value", 0.f);
    if (in.size() > 2 && in[2]) {
      if (!in[2]->is_const) return fail("Pad: constant value only");
      if (!in[2]->c.f.empty()) value = in[2]->c.f[0];
    }
    const size_t rk = xs.size();
    std::vector<int64_t> axes;
    if (in.size() > 3 && in[3]) {
      if (!in[3]->is_const) return fail("Pad: constant axes only");
      axes = in[3]->c.i;
    }
    std::vector<int64_t> pb(rk, 0), pe(rk, 0);
    if (axes.empty()) {
      if (pads.size() != 2 * rk) return fail("Pad: pads length");
      for (size_t d = 0; d < rk; ++d) { pb[d] = pads[d]; pe[d] = pads[d + rk]; }
    } else {
      if (pads.size() != 2 * axes.size()) return fail("Pad: pads length");
      for (size_t k = 0; k < axes.size(); ++k) {
        const int64_t a = axes[k] < 0 ? axes[k] + (int64_t)rk : axes[k];
        if (a < 0 || a >= (int64_t)rk) return fail("Pad: axis out of range");
        pb[a] = pads[k];
        pe[a] = pads[k + axes.size()];
      }
    }
    std::vector<int64_t> os(rk), start(rk);
    for (size_t d = 0; d < rk; ++d) {
      os[d] = xs[d] + pb[d] + pe[d];
      start[d] = -pb[d];
      if (os[d] < 0) return fail("Pad: negative pads remove more than the axis holds");
    }
    return plan_copy_out(nd.out[0], os, dptr(*in[0]), xs, start, std::vector<int64_t>(rk, 1), {}, value);
  }

  bool plan_concat(size_t ni, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    int64_t ax = nd.ai("axis", 0);
    const size_t rk = xs.size();
    if (ax < 0) ax += (int64_t)rk;
    std::vector<int64_t> os = xs;
    os[ax] = 0;
    for (Value* v : in) os[ax] += v->shape[ax];
    float* dst = make_out(nd.out[0], os);
    if (!dst) return false;
    const std::vector<int64_t> zero(rk, 0), one(rk, 1);
    int64_t off = 0;
    for (size_t q = 0; q < in.size(); ++q) {
      Value* v = in[q];
      std::vector<int64_t> doff(rk, 0);
      doff[ax] = off;
      off += v->shape[ax];
      auto direct = cat_patch.find(nd.in[q]);
      if (direct != cat_patch.end() && rk == 4 && ax == 1) {  // its producer writes it here
        for (auto& f : direct->second) f(dst + doff[1] * os[2] * os[3], (int)os[1]);
        if (up_pending.count(nd.in[q]))
          cat_up[nd.out[0]].push_back({nd.in[q], (int)doff[1], (int)(doff[1] + v->shape[1])});
        continue;
      }
      flush_up(nd.in[q]);
      if (q + 1 == in.size() && rk == 4 && ax == 1 && doff[1] % 32 == 0 && doff[1] > 0 && cat_tail_enabled()) {
        const int c = sole_consumer(nd.out[0], ni);
        if (c >= 0 && g.nodes[c].op == "Conv" && g.nodes[c].in[0] == nd.out[0]) {  // left to that Conv (cat_tail)
          const float* src = operand(*v);
          if (!src) return false;
          const std::vector<int64_t> vs = v->shape;
          cat_tail[nd.out[0]] = {src, (int)doff[1], (int)v->shape[1], [this, src, vs, dst, os, doff, zero, one]() {
                                   return plan_copy_into(src, vs, dst, os, vs, doff, zero, one, {}, 0.f);
                                 }};
          continue;
        }
      }
      if (!plan_copy_into(operand(*v), v->shape, dst, os, v->shape, doff, zero, one, {}, 0.f)) return false;
    }
    return true;
  }

  // a Split's axis and part sizes (split: the attribute's or the input's values, or null)
  bool split_sizes(const Node& nd, const std::vector<int64_t>& xs, const Value* split, int64_t* axis,
                   std::vector<int64_t>* sizes) {
    int64_t ax = nd.ai("axis", 0);
    if (ax < 0) ax += (int64_t)xs.size();
    std::vector<int64_t> sp = nd.ais("split");
    if (split) sp = split->c.i;
    const int64_t k = (int64_t)nd.out.size();
    if (sp.empty()) {
      // opset 18: ceil-sized parts, the last one smaller; before, even parts only
      if (xs[ax] % k != 0 && g.opset > 0 && g.opset < 18)
        return fail("Split '" + nd.name + "': uneven default split needs opset 18");
      const int64_t part = (xs[ax] + k - 1) / k;
      for (int64_t q = 0; q < k; ++q) sp.push_back(std::max<int64_t>(0, std::min(part, xs[ax] - q * part)));
    }
    int64_t sum = 0;
    for (int64_t v : sp) sum += v;
    if ((int64_t)sp.size() != k || sum != xs[ax]) return fail("Split '" + nd.name + "': sizes do not add up to the axis");
    *axis = ax;
    *sizes = sp;
    return true;
  }

  bool plan_split(size_t, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    const size_t rk = xs.size();
    int64_t ax = 0;
    std::vector<int64_t> sp;
    if (!split_sizes(nd, xs, in.size() > 1 ? in[1] : nullptr, &ax, &sp)) return false;
    const int64_t k = (int64_t)nd.out.size();
    int64_t off = 0;
    for (int64_t q = 0; q < k; ++q) {
      std::vector<int64_t> os = xs;
      os[ax] = sp[q];
      std::vector<int64_t> start(rk, 0);
      start[ax] = off;
      off += sp[q];
      if (!plan_copy_out(nd.out[q], os, dptr(*in[0]), xs, start, std::vector<int64_t>(rk, 1), {}, 0.f)) return false;
    }
    return true;
  }

  bool plan_slice(size_t, const Node& nd, Ins& in) {
    const std::vector<int64_t>& xs = in[0]->shape;
    const size_t rk = xs.size();
    std::vector<int64_t> st, en, axes, steps;
    if (in.size() >= 3) {
      for (size_t k = 1; k < in.size(); ++k)
        if (in[k] && !in[k]->is_const) return fail("Slice: constant starts/ends/axes/steps only");
      st = ints(*in[1]); en = ints(*in[2]);
      if (in.size() > 3 && in[3]) axes = ints(*in[3]);
      if (in.size() > 4 && in[4]) steps = ints(*in[4]);
    } else {
      st = nd.ais("starts"); en = nd.ais("ends"); axes = nd.ais("axes");
    }
    if (axes.empty()) for (size_t k = 0; k < st.size(); ++k) axes.push_back((int64_t)k);
    if (steps.empty()) steps.assign(st.size(), 1);
    std::vector<int64_t> os = xs, start(rk, 0), step(rk, 1);
    for (size_t k = 0; k < st.size(); ++k) {
      const int64_t a = axes[k] < 0 ? axes[k] + (int64_t)rk : axes[k];
      const int64_t L = xs[a], sk = steps[k];
      if (sk == 0) return fail("Slice: zero step");
      int64_t b = st[k] < 0 ? st[k] + L : st[k], e = en[k] < 0 ? en[k] + L : en[k];
      if (sk > 0) { b = std::clamp<int64_t>(b, 0, L); e = std::clamp<int64_t>(e, 0, L); os[a] = std::max<int64_t>(0, (e - b + sk - 1) / sk); }
      else { b = std::clamp<int64_t>(b, 0, L - 1); e = std::clamp<int64_t>(e, -1, L - 1); os[a] = std::max<int64_t>(0, (b - e - sk - 1) / (-sk)); }
      start[a] = b;
      step[a] = sk;
    }
    return plan_copy_out(nd.out[0], os, dptr(*in[0]), xs, start, step, {}, 0.f);
  }

  bool plan_resize(size_t, const Node& nd, Ins& in) {  // Resize, Upsample
    const std::string& op = nd.op;
    const std::vector<int64_t>& xs = in[0]->shape;
    if (xs.size() != 4) return fail(op + ": 4D only");
    std::vector<float> scales;
    std::vector<int64_t> sizes;
    if (op == "Upsample") {
      if (in.size() > 1 && in[1] && in[1]->is_const) scales = in[1]->c.f;
      else scales = nd.attrs.count("scales") ? nd.attrs.at("scales").fs : std::vector<float>{};
    } else {
      if (in.size() > 2 && in[2]) { if (!in[2]->is_const) return fail("Resize: constant scales only"); scales = in[2]->c.f; }
      if (in.size() > 3 && in[3]) { if (!in[3]->is_const) return fail("Resize: constant sizes only"); sizes = in[3]->c.i; }
    }
    ResizeParams p{};
    p.N = (int)xs[0]; p.C = (int)xs[1]; p.H = (int)xs[2]; p.W = (int)xs[3];
    if (!sizes.empty()) {
      if (sizes.size() != 4 || sizes[0] != xs[0] || sizes[1] != xs[1]) return fail("Resize: N, C must not change");
      p.Ho = (int)sizes[2]; p.Wo = (int)sizes[3];
      p.sy = (float)p.Ho / p.H; p.sx = (float)p.Wo / p.W;
    } else {
      if (scales.size() != 4 || scales[0] != 1.f || scales[1] != 1.f) return fail("Resize: scales on H, W only");
      p.sy = scales[2]; p.sx = scales[3];
      p.Ho = (int)std::floor(p.H * (double)p.sy);
      p.Wo = (int)std::floor(p.W * (double)p.sx);
    }
    const std::string mode = nd.as("mode", "nearest");
    if (mode != "nearest" && mode != "linear" && mode != "bilinear") return fail("Resize: mode " + mode);
    p.linear = mode != "nearest";
    // the position of `v` in `names`, or -1
    auto index_of = [](const std::string& v, std::initializer_list<const char*> names) {
      int k = 0;
      for (const char* n : names) { if (v == n) return k; ++k; }
      return -1;
    };
    const std::string ctm = nd.as("coordinate_transformation_mode", op == "Upsample" ? "asymmetric" : "half_pixel");
    p.ctm = index_of(ctm, {"half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric"});
    if (p.ctm < 0) return fail("Resize: coordinate_transformation_mode " + ctm);
    // Upsample (opset 7-9) has neither attribute: y[o] = x[floor(o / scale)]
    const std::string nm = nd.as("nearest_mode", op == "Upsample" ? "floor" : "round_prefer_floor");
    p.nearest = index_of(nm, {"round_prefer_floor", "round_prefer_ceil", "floor", "ceil"});
    if (p.nearest < 0) return fail("Resize: nearest_mode " + nm);
    if (nd.ai("antialias", 0) != 0) return fail("Resize: antialias is not supported");
    if (nd.has("axes")) return fail("Resize: axes is not supported");
    if (nd.as("keep_aspect_ratio_policy", "stretch") != "stretch")
      return fail("Resize: keep_aspect_ratio_policy " + nd.as("keep_aspect_ratio_policy", "") + " is not supported");
    p.x = dptr(*in[0]);
    if (head_up.count(nd.out[0]) && p.linear && p.Ho > 0 && p.Wo > 0 && (long)p.N * p.C * p.Ho * p.Wo < (1L << 31)) {
      Value v;  // no tensor yet: the class head reading it interpolates on the fly (or flush_head makes it)
      v.shape = {xs[0], xs[1], p.Ho, p.Wo};
      vals[nd.out[0]] = v;
      head_pending[nd.out[0]] = p;
      return true;
    }
    if (!(p.y = make_out(nd.out[0], {xs[0], xs[1], p.Ho, p.Wo}))) return false;
    if ((long)p.N * p.C * p.Ho * p.Wo >= (1L << 31)) return fail("Resize: output of 2^31 elements or more");
    std::shared_ptr<ResizeParams> pp;
    if (up_cand.count(nd.out[0]) && p.linear && (p.ctm == 0 || p.ctm == 1) && p.sy == 2.f && p.sx == 2.f &&
        p.Ho == 2 * p.H && p.Wo == 2 * p.W && p.C % 32 == 0 && s->conv_precision != PREC_F32)
      up_pending[nd.out[0]] = pp = std::make_shared<ResizeParams>(p);  // its consumer convolution computes it (or flush_up launches it)
    else
      pp = emit(resize_kernel_name(p), p, launch_resize);
    retarget_on_concat(nd.out[0], pp, p.C);
    return true;
  }

  // a following elementwise activation (the SE blocks' Relu / Sigmoid) in a
  // Gemm / MatMul's epilogue (PRelu not: its slope's axis is ambiguous on [M, N]);
  // then the launch
  // (last: the node whose output the launch writes so far — the MatMul, or the bias Add it absorbed)
  bool emit_gemm(size_t last, GemmParams& p, const std::vector<int64_t>& os, bool absorb_act) {
    std::string out = g.nodes[last].out[0];
    const int c1 = absorb_act && gemm_act_enabled() ? sole_consumer(out, last) : -1;
    if (c1 >= 0 && is_act(g.nodes[c1].op) && g.nodes[c1].op != "PRelu" && act_of(g.nodes[c1], &p.ep, p.N)) {
      done.insert((size_t)c1);
      out = g.nodes[c1].out[0];
    } else if (c1 < 0 && absorb_act && gemm_act_enabled()) {
      const int mul = act_pair(out, last, &p.ep);
      if (mul >= 0) {
        done.insert((size_t)mul);
        out = g.nodes[mul].out[0];
      }
    }
    if (!(p.y = make_out(out, os))) return false;
    emit(gemm_kernel_name(p), p, launch_gemm);
    return true;
  }

  bool plan_gemm(size_t ni, const Node& nd, Ins& in) {
    Value *a = in[0], *b = in[1];
    if (a->shape.size() != 2 || b->shape.size() != 2) return fail("Gemm: 2D operands");
    GemmParams p{};
    const bool ta = nd.ai("transA", 0) != 0, tb = nd.ai("transB", 0) != 0;
    p.alpha = nd.af("alpha", 1.f);
    p.beta = nd.af("beta", 1.f);
    p.batch = 1;
    p.M = (int)(ta ? a->shape[1] : a->shape[0]);
    p.K = (int)(ta ? a->shape[0] : a->shape[1]);
    p.N = (int)(tb ? b->shape[0] : b->shape[1]);
    if ((tb ? b->shape[1] : b->shape[0]) != p.K) return fail("Gemm: inner dimensions differ");
    p.sam = ta ? 1 : p.K; p.sak = ta ? p.M : 1;
    p.sbk = tb ? 1 : p.N; p.sbn = tb ? p.K : 1;
    if (in.size() > 2 && in[2]) {
      const std::vector<int64_t>& cs = in[2]->shape;
      if (cs.size() == 2) { p.scm = cs[0] == 1 ? 0 : cs[1]; p.scn = cs[1] == 1 ? 0 : 1; }
      else if (cs.size() == 1) { p.scm = 0; p.scn = cs[0] == 1 ? 0 : 1; }
      else { p.scm = 0; p.scn = 0; }
      p.c = operand(*in[2]);
    }
    p.a = operand(*a);
    p.b = operand(*b);
    if (!p.a || !p.b) return false;
    return emit_gemm(ni, p, {p.M, p.N}, true);
  }

  bool plan_matmul(size_t ni, const Node& nd, Ins& in) {
    Value *a = in[0], *b = in[1];
    const std::vector<int64_t>& as_ = a->shape;
    const std::vector<int64_t>& bs = b->shape;
    if (as_.size() < 2 || bs.size() < 2) return fail("MatMul: operands of rank >= 2 only");
    GemmParams p{};
    p.alpha = 1.f;
    p.beta = 1.f;
    p.M = (int)as_[as_.size() - 2]; p.K = (int)as_.back(); p.N = (int)bs.back();
    if (bs[bs.size() - 2] != p.K) return fail("MatMul: inner dimensions differ");
    int64_t ba = 1, bb = 1;
    for (size_t d = 0; d + 2 < as_.size(); ++d) ba *= as_[d];
    for (size_t d = 0; d + 2 < bs.size(); ++d) bb *= bs[d];
    if (bb != 1 && bb != ba) return fail("MatMul: batch broadcast beyond [B] x [1] not supported");
    p.batch = (int)ba;
    p.sab = (int64_t)p.M * p.K; p.sam = p.K; p.sak = 1;
    p.sbb = bb == 1 ? 0 : (int64_t)p.K * p.N; p.sbk = p.N; p.sbn = 1;
    std::vector<int64_t> os(as_.begin(), as_.end() - 2);
    os.push_back(p.M);
    os.push_back(p.N);
    p.a = operand(*a);
    if (b->is_const && p.sbb == 0) {
      // a constant B stored transposed ([N][K]): k contiguous for k_gemm<true>
      std::vector<float> bt((size_t)p.K * p.N);
      for (int k = 0; k < p.K; ++k)
        for (int n2 = 0; n2 < p.N; ++n2) bt[(size_t)n2 * p.K + k] = b->c.f[(size_t)k * p.N + n2];
      p.b = upload_vec(bt);
      p.sbk = 1; p.sbn = p.K;
    } else {
      p.b = operand(*b);
    }
    if (!p.a || !p.b) return false;
    // a Linear layer's bias: Add of a constant [N] (or [1, .., N]) that is all that reads the product
    size_t last = ni;
    const int ad = b->is_const ? sole_consumer(nd.out[0], ni) : -1;
    if (ad >= 0 && g.nodes[ad].op == "Add" && g.nodes[ad].in.size() == 2) {
      const Node& add = g.nodes[ad];
      Const tmp;
      const Const* bc = const_of(add.in[0] == nd.out[0] ? add.in[1] : add.in[0], &tmp);
      if (bc && !bc->is_int && bc->numel() == p.N && !bc->dims.empty() && bc->dims.back() == p.N &&
          bc->dims.size() <= os.size()) {
        if (!(p.c = upload_vec(bc->f))) return false;
        p.scm = 0; p.scn = 1;
        done.insert((size_t)ad);
        last = (size_t)ad;
      }
    }
    return emit_gemm(last, p, os, true);
  }

  // com.microsoft MatMulNBits (the q4 layers of a q4f16 export): Y = A @ W^T
  // (+ bias), W [N][K] dequantised once at create from 4-bit blocks:
  // W[n][k] = (q - zp) * scale[n][k / block_size], q the k-th nibble of row
  // n (low nibble first), zp the packed per-block zero point (default 8).
  bool plan_matmul_nbits(size_t ni, const Node& nd, Ins& in) {
    auto opt = [&](size_t k) { return in.size() > k ? in[k] : nullptr; };
    Value *a = in[0], *bq = opt(1), *sc = opt(2), *zp = opt(3), *gidx = opt(4), *bias = opt(5);
    if (!bq || !bq->is_const || !sc || !sc->is_const || (zp && !zp->is_const) || (bias && !bias->is_const))
      return fail("MatMulNBits '" + nd.name + "': B, scales, zero_points and bias must be initializers");
    if (gidx) return fail("MatMulNBits '" + nd.name + "': g_idx is not supported");
    const int64_t K = nd.ai("K", 0), N = nd.ai("N", 0), bits = nd.ai("bits", 4), bs = nd.ai("block_size", 0);
    if (bits != 4 || bs < 16 || K <= 0 || N <= 0) return fail("MatMulNBits '" + nd.name + "': 4-bit blocks only");
    const int64_t kb = (K + bs - 1) / bs, blob = bs * bits / 8, zpb = (kb * bits + 7) / 8;
    if (bq->c.numel() != N * kb * blob || sc->c.numel() != N * kb)
      return fail("MatMulNBits '" + nd.name + "': B / scales sizes do not match K, N, block_size");
    if (zp && (!zp->c.is_int || zp->c.numel() != N * zpb))
      return fail("MatMulNBits '" + nd.name + "': only packed uint8 zero points are supported");
    if (a->shape.empty() || a->shape.back() != K) return fail("MatMulNBits '" + nd.name + "': A's last dim is not K");
    std::vector<float> w((size_t)(N * K));
    for (int64_t n = 0; n < N; ++n)
      for (int64_t b = 0; b < kb; ++b) {
        const double sv = sc->c.f[n * kb + b];
        const int z = zp ? (int)((zp->c.i[n * zpb + b / 2] >> ((b & 1) * 4)) & 15) : 8;
        for (int64_t j = 0; j < bs && b * bs + j < K; ++j) {
          const int q = (int)((bq->c.i[(n * kb + b) * blob + j / 2] >> ((j & 1) * 4)) & 15);
          float v = (float)((double)(q - z) * sv);
          if (sc->c.f16) v = round_half(v);
          w[n * K + b * bs + j] = v;
        }
      }
    GemmParams p{};
    p.alpha = 1.f;
    p.beta = 1.f;
    p.batch = 1;
    p.K = (int)K;
    p.N = (int)N;
    p.M = (int)(a->numel() / K);
    p.sam = K; p.sak = 1;
    p.sbn = K; p.sbk = 1;  // W stored [N][K]
    p.a = operand(*a);
    p.b = upload_vec(w);
    if (bias) {
      if (bias->c.numel() != N) return fail("MatMulNBits '" + nd.name + "': bias must have N elements");
      p.c = operand(*bias);
      p.scm = 0; p.scn = 1;
    }
    if (!p.a || !p.b || (bias && !p.c)) return false;
    std::vector<int64_t> os(a->shape.begin(), a->shape.end() - 1);
    os.push_back(N);
    return emit_gemm(ni, p, os, false);
  }

  // ---- fused attention (vso_attn.hip) --------------------------------------
  //   MatMul(Q, Transpose(K: last two axes swapped)) [-> Mul | Div by a constant
  //   scalar] [-> Add(bias)] -> Softmax(last axis) -> MatMul(., V)
  // every interior value read by the next node only; a Mul by a constant
  // scalar in front of the first MatMul, on Q or on K, read by that MatMul
  // only, is part of it.  Found by structure before the walk (find_attention):
  // the nodes ahead of the second MatMul are done from there on and that
  // MatMul stands for the pattern.  Its plan (try_plan_attn) sees the shapes:
  // Q, K, V runtime tensors with equal leading dims, d and dv multiples of 4 up
  // to kAttnMaxD, a bias whose last two dims are [Nq, Nk] and whose leading ones
  // are 1 or Q's.  Anything else: the nodes get today's launches, in order.
  struct AttnFuse {
    std::vector<size_t> pre;  // the nodes ahead of the second MatMul, in node order (a shared Transpose not among them)
    std::string q, k, v, bias;  // k: the Transpose's input
    double scale;
  };
  std::map<size_t, AttnFuse> attn;  // by the second MatMul (find_attention)

  // `name` = Mul(t, constant scalar) read by node `by` only: t and the scalar
  bool scaled_operand(const std::string& name, int by, std::string* t, double* c, int* node) {
    const int p = producer(name);
    if (p < 0 || g.nodes[p].op != "Mul" || g.nodes[p].in.size() != 2 || sole_consumer(name, (size_t)p) != by) return false;
    for (int side = 0; side < 2; ++side)
      if (scalar_of(g.nodes[p].in[1 - side], c)) {
        *t = g.nodes[p].in[side];
        *node = p;
        return true;
      }
    return false;
  }

  void find_attention() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& m1 = g.nodes[k];
      if (m1.op != "MatMul" || m1.in.size() != 2 || done.count(k)) continue;
      AttnFuse f;
      f.scale = 1.0;
      f.q = m1.in[0];
      std::string kt = m1.in[1], t;
      double c;
      int node;
      if (scaled_operand(f.q, (int)k, &t, &c, &node)) { f.q = t; f.scale *= c; f.pre.push_back((size_t)node); }
      if (scaled_operand(kt, (int)k, &t, &c, &node)) { kt = t; f.scale *= c; f.pre.push_back((size_t)node); }
      const int tr = producer(kt);
      if (tr < 0 || g.nodes[tr].op != "Transpose") continue;
      const std::vector<int64_t> perm = g.nodes[tr].ais("perm");
      const size_t rk = perm.size();
      bool swap = rk >= 2;
      for (size_t a = 0; swap && a < rk; ++a) swap = perm[a] == (int64_t)(a + 2 < rk ? a : a + 2 == rk ? rk - 1 : rk - 2);
      if (!swap) continue;
      f.k = g.nodes[tr].in[0];
      // (read by the pattern only: no launch; else the Transpose stays and the fused node reads its input all the same)
      const int tc = sole_consumer(kt, (size_t)tr);
      if (tc == (int)k || (tc >= 0 && !f.pre.empty() && tc == (int)f.pre.back())) f.pre.push_back((size_t)tr);
      f.pre.push_back(k);
      std::string cur = m1.out[0];
      int nx = sole_consumer(cur, k);
      if (nx >= 0 && (g.nodes[nx].op == "Mul" || g.nodes[nx].op == "Div") && with_scalar(g.nodes[nx], cur, &c)) {
        f.scale = g.nodes[nx].op == "Mul" ? f.scale * c : f.scale / c;
        f.pre.push_back((size_t)nx);
        cur = g.nodes[nx].out[0];
        nx = sole_consumer(cur, (size_t)nx);
      }
      if (nx >= 0 && g.nodes[nx].op == "Add" && g.nodes[nx].in.size() == 2 && g.nodes[nx].in[0] != g.nodes[nx].in[1]) {
        f.bias = g.nodes[nx].in[0] == cur ? g.nodes[nx].in[1] : g.nodes[nx].in[0];
        f.pre.push_back((size_t)nx);
        cur = g.nodes[nx].out[0];
        nx = sole_consumer(cur, (size_t)nx);
      }
      if (nx < 0 || g.nodes[nx].op != "Softmax") continue;
      int64_t ax = g.nodes[nx].ai("axis", g.opset > 0 && g.opset < 13 ? 1 : -1);
      if (ax < 0) ax += (int64_t)rk;
      if (ax != (int64_t)rk - 1) continue;
      f.pre.push_back((size_t)nx);
      cur = g.nodes[nx].out[0];
      const int m2 = sole_consumer(cur, (size_t)nx);
      if (m2 < 0 || g.nodes[m2].op != "MatMul" || g.nodes[m2].in.size() != 2 || g.nodes[m2].in[0] != cur ||
          g.nodes[m2].in[1] == cur)
        continue;
      f.v = g.nodes[m2].in[1];
      bool taken = done.count((size_t)m2) != 0;
      for (size_t q : f.pre) taken = taken || done.count(q);
      if (taken) continue;
      std::sort(f.pre.begin(), f.pre.end());
      for (size_t q : f.pre) done.insert(q);
      attn[(size_t)m2] = f;
    }
  }

  // The second MatMul `ni` of an attention pattern as one k_attn launch.  1:
  // planned; 0: not this shape class — the nodes ahead got their own launches
  // and `ni` goes to plan_matmul; -1: an error.
  int try_plan_attn(size_t ni) {
    const AttnFuse f = attn[ni];
    attn.erase(ni);
    auto decline = [&]() {
      for (size_t q : f.pre)
        if (!plan_node(q)) return -1;
      return 0;
    };
    Value *q = val(f.q), *k = val(f.k), *v = val(f.v), *bias = f.bias.empty() ? nullptr : val(f.bias);
    if (!q || !k || !v || q->is_const || k->is_const || v->is_const || (!f.bias.empty() && !bias)) return decline();
    const std::vector<int64_t>&qs = q->shape, &ks = k->shape, &vs = v->shape;
    const size_t rk = qs.size();
    if (rk < 2 || rk > (size_t)kMaxDims || ks.size() != rk || vs.size() != rk) return decline();
    AttnParams p{};
    int64_t bh = 1;
    for (size_t a = 0; a + 2 < rk; ++a) {
      if (ks[a] != qs[a] || vs[a] != qs[a]) return decline();
      bh *= qs[a];
      p.lead[a] = (int)qs[a];
    }
    p.nlead = (int)rk - 2;
    const int64_t Nq = qs[rk - 2], d = qs[rk - 1], Nk = ks[rk - 2], dv = vs[rk - 1];
    if (ks[rk - 1] != d || vs[rk - 2] != Nk || bh < 1 || Nq < 1 || Nk < 1 || bh * Nq * std::max(d, dv) >= (1LL << 31) ||
        bh * Nk * std::max(d, dv) >= (1LL << 31) || !std::isfinite(f.scale))
      return decline();
    if (bias) {
      const std::vector<int64_t>& bs = bias->shape;
      const size_t rb = bs.size();
      if (rb < 2 || rb > rk || bs[rb - 2] != Nq || bs[rb - 1] != Nk) return decline();
      std::vector<int64_t> st;
      fill_strides(bs, &st);
      for (size_t a = 0; a + 2 < rb; ++a) {
        const size_t qa = a + rk - rb;
        if (bs[a] != 1 && bs[a] != qs[qa]) return decline();
        p.bstr[qa] = bs[a] == 1 ? 0 : st[a];
      }
    }
    p.BH = (int)bh; p.Nq = (int)Nq; p.Nk = (int)Nk; p.d = (int)d; p.dv = (int)dv;
    p.scale = (float)f.scale;
    for (const std::string* n : {&f.q, &f.k, &f.v, &f.bias})
      if (!n->empty()) flush_input(*n);
    p.q = dptr(*q); p.k = dptr(*k); p.v = dptr(*v);
    if (bias && !(p.bias = operand(*bias))) return -1;
    std::vector<int64_t> os(qs.begin(), qs.end() - 1);
    os.push_back(dv);
    // (a placeholder output for the support test: the real one is made once the plan is taken)
    p.y = dptr(*q);
    if (!attn_supported(p)) return decline();
    if (!(p.y = make_out(g.nodes[ni].out[0], os))) return -1;
    emit(attn_kernel_name(p), p, launch_attn);
    s->attn_nodes++;
    return 1;
  }

  // ---- statically quantised (QDQ) graphs (vso_quant.hip) -------------------
  // QuantizeLinear of a runtime f32 tensor gives a quantised runtime tensor
  // (Value::qtype; one byte per element, its buffer a quarter of the floats);
  // DequantizeLinear of one gives f32 again: k_quantize / k_dequantize, and
  // between them the float kernels — the plan that always works.  Three
  // patterns run on the integers instead, one launch each (find_qdq), every
  // interior value read by the next node only:
  //   DequantizeLinear(xq) -> Conv(., DequantizeLinear(Wq const), [B]) [-> Relu
  //   | Clip] -> QuantizeLinear: k_qconv_tile (group 1) or k_qconv_dw (depthwise);
  //   Add(DequantizeLinear(a), DequantizeLinear(b)) [-> Relu] -> QuantizeLinear
  //   of equal shapes: k_qadd.
  // Nothing else may read a quantised tensor.  A quantised graph output is
  // written out as the exact integers in float32 (a k_dequantize of scale 1,
  // zero point 0, launched where the tensor is produced).
  struct QParams {
    float scale = 1.f;
    int zp = 0;
    int type = DT_UINT8;  // DT_UINT8 / DT_INT8
    bool has_zp = false;
    int qmin() const { return type == DT_INT8 ? -128 : 0; }
    int qmax() const { return type == DT_INT8 ? 127 : 255; }
  };
  // scale and zero point of a Quantize / DequantizeLinear node over a runtime
  // tensor: constants of one element each, uint8 / int8; else *why says what
  // is refused
  bool q_params(const Node& nd, QParams* q, std::string* why) {
    const std::string at = nd.op + " '" + nd.name + "': unsupported: ";
    Const ts, tz;
    const Const* sc = nd.in.size() > 1 ? const_of(nd.in[1], &ts) : nullptr;
    if (!sc) return *why = at + "the scale of a runtime tensor must be a constant", false;
    const bool has_zp = nd.in.size() > 2 && !nd.in[2].empty();
    const Const* zp = has_zp ? const_of(nd.in[2], &tz) : nullptr;
    if (has_zp && !zp) return *why = at + "the zero point of a runtime tensor must be a constant", false;
    if (sc->numel() != 1 || (zp && zp->numel() != 1) || nd.ai("block_size", 0) != 0)
      return *why = at + "a runtime tensor is quantised per tensor only (one scale, one zero point)", false;
    if (sc->is_int || sc->f16 || sc->f.empty() || !(sc->f[0] > 0.f) || !std::isfinite(sc->f[0]))
      return *why = at + "a positive float32 scale only", false;
    q->scale = sc->f[0];
    q->has_zp = zp != nullptr;
    if (zp) {
      if (!zp->is_int || (zp->dtype != DT_UINT8 && zp->dtype != DT_INT8))
        return *why = at + "runtime tensors of uint8 and int8 only (zero point of type " + std::to_string(zp->dtype) + ")", false;
      q->type = zp->dtype;
      q->zp = (int)zp->i[0];
    }
    if (nd.op == "QuantizeLinear" && !zp) {
      const int64_t od = nd.ai("output_dtype", 0);
      if (od != 0 && od != DT_UINT8 && od != DT_INT8)
        return *why = at + "runtime tensors of uint8 and int8 only (output_dtype " + std::to_string(od) + ")", false;
      if (od) q->type = (int)od;
    }
    if (nd.ai("saturate", 1) != 1) return *why = at + "saturate 1 only", false;
    return true;
  }

  static bool qdq_enabled() { static const bool on = env_on("VSO_QDQ"); return on; }

  // a new quantised runtime tensor (null: err set); a graph output also gets its float32 form
  std::map<std::string, int> q_out;  // quantised graph outputs: the float32 buffer holding the exact integers
  bool is_graph_output(const std::string& name) const {
    for (const IO& o : g.outputs)
      if (o.name == name) return true;
    return false;
  }
  unsigned char* make_q_out(const std::string& name, const std::vector<int64_t>& shape, int type) {
    Value v;
    v.shape = shape;
    v.qtype = type;
    if (v.numel() >= (int64_t{1} << 30)) return fail("quantised tensor '" + name + "': 2^30 elements or more"), nullptr;
    if ((v.buf = new_buf(type == DT_INT32 ? v.numel() : (v.numel() + 3) / 4)) < 0) return nullptr;
    vals[name] = v;
    return reinterpret_cast<unsigned char*>(s->bufs[v.buf]);
  }
  const unsigned char* qptr(const Value& v) { return reinterpret_cast<const unsigned char*>(s->bufs[v.buf]); }
  // after the launch producing quantised `name`: its float32 form when it is a graph output
  bool q_publish(const std::string& name) {
    if (!is_graph_output(name)) return true;
    const Value& v = vals[name];
    const int b = new_buf(v.numel());
    if (b < 0) return false;
    emit("vso::k_dequantize(vso::DequantParams)",
         DequantParams{qptr(v), s->bufs[b], (long)v.numel(), 1.f, 0, v.qtype == DT_INT8}, launch_dequantize);
    q_out[name] = b;
    return true;
  }

  bool plan_quantize(size_t, const Node& nd, Ins& in) {
    QParams q;
    if (!q_params(nd, &q, &err)) return false;
    Value& x = *in[0];
    if (x.is_const || x.qtype) return fail(nd.op + " '" + nd.name + "': unsupported: a runtime float32 input only");
    const float* xp = dptr(x);
    const long n = (long)x.numel();
    unsigned char* y = make_q_out(nd.out[0], x.shape, q.type);
    if (!y) return false;
    emit("vso::k_quantize(vso::QuantParams)", QuantParams{xp, y, n, q.scale, q.zp, q.qmin(), q.qmax()}, launch_quantize);
    return q_publish(nd.out[0]);
  }

  // DequantizeLinear of a runtime tensor (of constants: folded on the host, vso_fold.cpp)
  bool plan_dequantize(size_t, const Node& nd, Ins& in) {
    Value& x = *in[0];
    if (x.is_const) return fail("DequantizeLinear '" + nd.name + "': unsupported: a constant input with a runtime scale");
    if (!x.qtype)
      return fail("DequantizeLinear '" + nd.name + "': unsupported: its runtime input is not a quantised tensor");
    QParams q;
    if (!q_params(nd, &q, &err)) return false;
    if (q.has_zp && q.type != x.qtype)
      return fail("DequantizeLinear '" + nd.name + "': unsupported: the zero point's type differs from the input's");
    const unsigned char* xp = qptr(x);
    const long n = (long)x.numel();
    const int sgn = x.qtype == DT_INT8;
    const std::vector<int64_t> shape = x.shape;
    float* y = make_out(nd.out[0], shape);
    if (!y) return false;
    emit("vso::k_dequantize(vso::DequantParams)", DequantParams{xp, y, n, q.scale, q.zp, sgn}, launch_dequantize);
    return true;
  }

  // Only DequantizeLinear (and ConvInteger / MatMulInteger as input 0) may read a QuantizeLinear's output — its
  // buffer is a quarter of the floats — whichever plan its reader ends up in: checked on the graph, ahead of the
  // pre-passes that absorb nodes into other launches
  // The dynamic form's tensors alike: a DynamicQuantizeLinear's y is read by DequantizeLinear or as input 0 of
  // ConvInteger / MatMulInteger, its zero point as their input 2 only; their int32 output by Cast to FLOAT only,
  // and it is no graph output (the outputs leave as float32, which cannot hold it)
  bool check_quantised_readers() {
    std::set<std::string> q, dy, dz, i32;
    for (const Node& nd : g.nodes) {
      if (nd.op == "QuantizeLinear" && !nd.out.empty()) q.insert(nd.out[0]);
      if (nd.op == "DynamicQuantizeLinear") {
        if (!nd.out.empty() && !nd.out[0].empty()) dy.insert(nd.out[0]);
        if (nd.out.size() > 2 && !nd.out[2].empty()) dz.insert(nd.out[2]);
      }
      if ((nd.op == "ConvInteger" || nd.op == "MatMulInteger") && !nd.out.empty()) i32.insert(nd.out[0]);
    }
    if (q.empty() && dy.empty() && i32.empty()) return true;
    for (const Node& nd : g.nodes) {
      const bool integer = nd.op == "ConvInteger" || nd.op == "MatMulInteger";
      const std::string at = nd.op + " '" + nd.name + "': unsupported: ";
      for (size_t k = 0; k < nd.in.size(); ++k) {
        if (q.count(nd.in[k]) && !((nd.op == "DequantizeLinear" || integer) && k == 0))
          return fail(at + "a quantised tensor is read by DequantizeLinear only");
        if (dy.count(nd.in[k]) && !((nd.op == "DequantizeLinear" || integer) && k == 0))
          return fail(at + "a dynamically quantised tensor is read by ConvInteger, MatMulInteger (input 0) and DequantizeLinear only");
        if (dz.count(nd.in[k]) && !(integer && k == 2))
          return fail(at + "a DynamicQuantizeLinear's zero point is read by ConvInteger and MatMulInteger (input 2) only");
        if (i32.count(nd.in[k]) && !(nd.op == "Cast" && k == 0 && nd.ai("to", DT_FLOAT) == DT_FLOAT))
          return fail(at + "an int32 tensor is read by Cast to FLOAT only");
      }
    }
    for (const IO& o : g.outputs)
      if (i32.count(o.name))
        return fail("graph output '" + o.name + "': unsupported: an int32 tensor (ConvInteger, MatMulInteger) is no graph "
                    "output: Cast it to FLOAT");
    return true;
  }

  struct QFuse {
    int kind;         // 0 k_qconv_tile, 1 k_qconv_dw, 2 k_qadd
    int dq_a, dq_b;   // the DequantizeLinear nodes of the runtime operands (dq_b: k_qadd)
    int dq_w;         // the constant weights' DequantizeLinear
    int act, q;       // the Relu / Clip (-1: none) and the QuantizeLinear
  };
  std::map<size_t, QFuse> qfuse;  // by Conv / Add node (find_qdq)

  // `name` is DequantizeLinear of a runtime tensor, read by node `by` only: that node, or -1
  int runtime_dq(const std::string& name, size_t by) {
    const int p = producer(name);
    if (p < 0 || g.nodes[p].op != "DequantizeLinear" || g.nodes[p].in.empty() || done.count((size_t)p)) return -1;
    Const t;
    QParams q;
    std::string why;
    if (const_of(g.nodes[p].in[0], &t) || !q_params(g.nodes[p], &q, &why)) return -1;
    return sole_consumer(name, (size_t)p) == (int)by ? p : -1;
  }
  // the constant weights of a fused Conv: int8 / uint8 [M][Cg][kh][kw], scale and zero point per tensor or per
  // output channel (axis 0), Wq - zw within int8 -> wi [M][Cg * kh * kw], sw [M]
  bool q_weights(const Node& dq, std::vector<signed char>* wi, std::vector<float>* sw) {
    Const t0, t1, t2;
    const Const* w = dq.in.size() > 1 ? const_of(dq.in[0], &t0) : nullptr;
    const Const* sc = w ? const_of(dq.in[1], &t1) : nullptr;
    const bool has_zp = dq.in.size() > 2 && !dq.in[2].empty();
    const Const* zp = has_zp && sc ? const_of(dq.in[2], &t2) : nullptr;
    if (!w || !sc || (has_zp && !zp) || !w->is_int || (w->dtype != DT_INT8 && w->dtype != DT_UINT8) ||
        w->dims.size() != 4 || sc->is_int || sc->f16 || dq.ai("block_size", 0) != 0)
      return false;
    const int64_t M = w->dims[0], per = w->numel() / std::max<int64_t>(M, 1), ns = sc->numel();
    if (M < 1 || (ns != 1 && (ns != M || dq.ai("axis", 1) != 0)) || (zp && (zp->numel() != ns || !zp->is_int))) return false;
    wi->resize((size_t)w->numel());
    sw->resize((size_t)M);
    for (int64_t m = 0; m < M; ++m) {
      (*sw)[m] = sc->f[ns == 1 ? 0 : m];
      const int64_t z = zp ? zp->i[ns == 1 ? 0 : m] : 0;
      for (int64_t k = 0; k < per; ++k) {
        const int64_t v = w->i[m * per + k] - z;
        if (v < -128 || v > 127) return false;
        (*wi)[m * per + k] = (signed char)v;
      }
    }
    return true;
  }
  bool const_known(const std::string& n) {
    Const t;
    return const_of(n, &t) != nullptr;
  }
  // [-> Relu | Clip(constant bounds)] -> QuantizeLinear behind `out` (written by node `last`), each read once
  bool q_tail(const std::string& out, size_t last, bool clip_ok, int* act, int* q) {
    int c = sole_consumer(out, last);
    *act = -1;
    if (c >= 0 && (g.nodes[c].op == "Relu" || (clip_ok && g.nodes[c].op == "Clip")) && g.nodes[c].in[0] == out) {
      const Node& a = g.nodes[c];
      for (size_t k = 1; k < a.in.size(); ++k)
        if (!a.in[k].empty() && !const_known(a.in[k])) return false;
      *act = c;
      c = sole_consumer(a.out[0], (size_t)c);
    }
    if (c < 0 || g.nodes[c].op != "QuantizeLinear" || g.nodes[c].in.empty()) return false;
    if (g.nodes[c].in[0] != (*act >= 0 ? g.nodes[*act].out[0] : out)) return false;
    QParams qp;
    std::string why;
    if (!q_params(g.nodes[c], &qp, &why)) return false;
    *q = c;
    return true;
  }

  void find_qdq() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& nd = g.nodes[k];
      if (done.count(k) || nd.out.empty()) continue;
      QFuse f{0, -1, -1, -1, -1, -1};
      if (nd.op == "Conv" && nd.in.size() >= 2) {
        f.dq_a = runtime_dq(nd.in[0], k);
        f.dq_w = producer(nd.in[1]);
        if (f.dq_a < 0 || f.dq_w < 0 || g.nodes[f.dq_w].op != "DequantizeLinear") continue;
        std::vector<signed char> wi;
        std::vector<float> sw;
        if (!q_weights(g.nodes[f.dq_w], &wi, &sw)) continue;
        Const t;
        const Const* w = const_of(g.nodes[f.dq_w].in[0], &t);
        const int64_t G = nd.ai("group", 1), M = w->dims[0];
        // (one channel to one channel is both: the depthwise form where it has the shape)
        if (G == M && w->dims[1] == 1 && w->dims[2] <= 7 && w->dims[3] <= 7) f.kind = 1;
        else if (G == 1) f.kind = 0;
        else continue;
        if (nd.in.size() > 2 && !nd.in[2].empty() && !const_known(nd.in[2])) {  // a float constant, or DequantizeLinear of one
          const int pb = producer(nd.in[2]);
          bool ok = pb >= 0 && g.nodes[pb].op == "DequantizeLinear";
          for (size_t q = 0; ok && q < g.nodes[pb].in.size(); ++q)
            ok = g.nodes[pb].in[q].empty() || const_known(g.nodes[pb].in[q]);
          if (!ok) continue;
        }
        if (!q_tail(nd.out[0], k, true, &f.act, &f.q)) continue;
      } else if (nd.op == "Add" && nd.in.size() == 2 && nd.in[0] != nd.in[1]) {
        f.kind = 2;
        f.dq_a = runtime_dq(nd.in[0], k);
        f.dq_b = runtime_dq(nd.in[1], k);
        if (f.dq_a < 0 || f.dq_b < 0 || !q_tail(nd.out[0], k, false, &f.act, &f.q)) continue;
      } else {
        continue;
      }
      for (int q : {f.dq_a, f.dq_b, f.act, f.q})
        if (q >= 0) done.insert((size_t)q);
      qfuse[k] = f;
    }
  }

  // the pattern cannot run fused after all (shapes, sizes): its DequantizeLinear nodes get their launches now,
  // the activation and the QuantizeLinear theirs when the walk reaches them
  int q_unfuse(const QFuse& f) {
    for (int q : {f.act, f.q})
      if (q >= 0) done.erase((size_t)q);
    for (int q : {f.dq_a, f.dq_b})
      if (q >= 0 && !plan_node((size_t)q)) return -1;
    return 0;
  }

  // false: the QuantizeLinear's constants or the Clip's bounds are not values yet (a Constant node placed behind
  // the pattern's head): the caller leaves the pattern unfused
  bool q_requant(const QFuse& f, int channels, Requant* rq, int* type) {
    QParams q;
    std::string why;
    if (!q_params(g.nodes[f.q], &q, &why)) return false;
    Epilogue ep{};
    if (f.act >= 0 && !act_of(g.nodes[f.act], &ep, channels)) return false;
    *rq = Requant{q.scale, q.zp, q.qmin(), q.qmax(), ep.act, ep.a0, ep.a1};
    *type = q.type;
    return true;
  }

  // the node heading a pattern of find_qdq: 1 planned as one launch, 0 left to the nodes as they are, -1 failed
  int try_plan_q(size_t ni) {
    const QFuse f = qfuse[ni];
    qfuse.erase(ni);
    const Node& nd = g.nodes[ni];
    const Node& da = g.nodes[f.dq_a];
    Value* a = val(da.in[0]);
    QParams qa, qb;
    std::string why;
    if (!a || a->is_const || !a->qtype || !q_params(da, &qa, &why) || (qa.has_zp && qa.type != a->qtype)) return q_unfuse(f);
    const int asgn = a->qtype == DT_INT8;
    if (f.kind == 2) {
      const Node& db = g.nodes[f.dq_b];
      Value* b = val(db.in[0]);
      if (!b || b->is_const || !b->qtype || !q_params(db, &qb, &why) || (qb.has_zp && qb.type != b->qtype) ||
          b->shape != a->shape)
        return q_unfuse(f);
      QAddParams p{};
      int type;
      if (!q_requant(f, 0, &p.rq, &type)) return q_unfuse(f);
      p.a = qptr(*a);
      p.b = qptr(*b);
      p.n = (long)a->numel();
      p.sa = qa.scale; p.sb = qb.scale; p.za = qa.zp; p.zb = qb.zp;
      p.asgn = asgn; p.bsgn = b->qtype == DT_INT8;
      const std::string& out = g.nodes[f.q].out[0];
      const std::vector<int64_t> shape = a->shape;
      if (!(p.y = make_q_out(out, shape, type))) return -1;
      emit("vso::k_qadd(vso::QAddParams)", p, launch_qadd);
      s->qconv_nodes++;
      return q_publish(out) ? 1 : -1;
    }
    // the Conv's geometry from the quantised tensor's shape (the DequantizeLinear's output has no tensor)
    Value ph;
    ph.shape = a->shape;
    vals[da.out[0]] = ph;
    ConvPlan c;
    if (!conv_geometry(nd, &c)) return -1;
    const ConvParams& cp = c.p;
    std::vector<signed char> wi;
    std::vector<float> sw;
    if (!q_weights(g.nodes[f.dq_w], &wi, &sw)) return fail("internal: the weights of a quantised Conv"), -1;
    const bool dw = f.kind == 1 && !(cp.G == 1 && ((cp.sh != 1 && cp.sh != 2) || (cp.sw != 1 && cp.sw != 2)));
    QConvParams p{};
    int type;
    // (sizes: 32-bit indices with room for a grid stride; K: |x| |w| <= 2^14 per term, so the int32 accumulator
    // and zero-point correction hold below 2^16 terms)
    if (!q_requant(f, cp.M, &p.rq, &type) || (int64_t)cp.Cg * cp.kh * cp.kw >= (1 << 16) ||
        (int64_t)cp.N * cp.C * cp.H * cp.W >= (int64_t{1} << 30) || (int64_t)cp.N * cp.M * cp.Ho * cp.Wo >= (int64_t{1} << 30) ||
        (dw && (cp.G != cp.C || cp.Cg != 1 || (cp.sh != 1 && cp.sh != 2) || (cp.sw != 1 && cp.sw != 2))) ||
        (!dw && cp.G != 1)) {
      vals.erase(da.out[0]);
      return q_unfuse(f);
    }
    p.N = cp.N; p.C = cp.C; p.H = cp.H; p.W = cp.W; p.M = cp.M; p.Ho = cp.Ho; p.Wo = cp.Wo;
    p.kh = cp.kh; p.kw = cp.kw; p.sh = cp.sh; p.sw = cp.sw; p.dh = cp.dh; p.dw = cp.dw; p.pt = cp.pt; p.pl = cp.pl;
    p.K = cp.Cg * cp.kh * cp.kw;
    std::vector<float> mult((size_t)cp.M);
    for (int m = 0; m < cp.M; ++m) mult[m] = qa.scale * sw[m];
    if (!(p.mult = upload_vec(mult))) return -1;
    if (c.has_bias && !(p.bias = upload_vec(c.bias))) return -1;
    if (dw) {
      p.zx = qa.zp;
      p.xsgn = asgn;
      if (!(p.w = static_cast<const signed char*>(upload_bytes(wi.data(), wi.size())))) return -1;
    } else {
      // signed operands: a uint8 activation is read as xq - 128 with the zero point zx - 128
      const int zxs = asgn ? qa.zp : qa.zp - 128;
      p.xflip = asgn ? 0 : 0x80;
      p.xpad = zxs & 0xff;
      p.Kp = (p.K + kQK - 1) / kQK * kQK;
      p.Mp = (p.M + kQBM - 1) / kQBM * kQBM;
      std::vector<signed char> packed((size_t)p.Mp * p.Kp, 0);
      std::vector<int> corr((size_t)p.M);
      for (int m = 0; m < p.M; ++m) {
        int sum = 0;
        for (int k = 0; k < p.K; ++k) {
          packed[(size_t)m * p.Kp + k] = wi[(size_t)m * p.K + k];
          sum += wi[(size_t)m * p.K + k];
        }
        corr[m] = zxs * sum;
      }
      if (!(p.w = static_cast<const signed char*>(upload_bytes(packed.data(), packed.size())))) return -1;
      if (!(p.corr = static_cast<const int*>(upload_bytes(corr.data(), corr.size() * 4)))) return -1;
    }
    p.x = qptr(*a);
    const std::string& out = g.nodes[f.q].out[0];
    if (!(p.y = make_q_out(out, c.oshape, type))) return -1;
    if (dw) emit("vso::k_qconv_dw(vso::QConvParams)", p, launch_qconv_dw);
    else emit("vso::k_qconv_tile(vso::QConvParams)", p, launch_qconv_tile);
    s->qconv_nodes++;
    return q_publish(out) ? 1 : -1;
  }

  // ---- dynamically quantised graphs (vso_dynq.hip) --------------------------
  // What onnxruntime's quantize_dynamic writes.  DynamicQuantizeLinear of a
  // runtime f32 tensor: two launches (k_dyn_minmax, k_dyn_quantize) giving a
  // uint8 byte tensor, y_scale (a rank-0 float32 runtime tensor) and
  // y_zero_point (a one-element byte tensor), all three in HBM.  ConvInteger /
  // MatMulInteger of a byte tensor by constant weights: one launch giving an
  // int32 runtime tensor (Value::qtype DT_INT32), which only Cast to FLOAT
  // reads — the plan that always works.  find_dynq finds the chain
  //   ConvInteger | MatMulInteger -> Cast(FLOAT) -> Mul(., s) [-> Add(constant
  //   bias)] [-> Relu | Clip(constant bounds)],  s = Mul(x_scale, w_scale)
  // every interior value and s read by the next node only: one launch with the
  // float epilogue (the same roundings, so the same bits), the scalar Mul none.
  static bool dynq_enabled() { static const bool on = env_on("VSO_DYNQ"); return on; }

  bool plan_dynamic_quantize(size_t ni, const Node& nd, Ins& in) {
    const std::string at = "DynamicQuantizeLinear '" + nd.name + "': unsupported: ";
    if (in.empty() || !in[0] || in[0]->is_const || in[0]->qtype) return fail(at + "a runtime float32 input only");
    if (nd.out.size() != 3) return fail(at + "three outputs only");
    DynQParams p{};
    p.x = dptr(*in[0]);
    p.n = (long)in[0]->numel();
    const std::vector<int64_t> shape = in[0]->shape;
    std::string names[3];
    for (int k = 0; k < 3; ++k) names[k] = nd.out[k].empty() ? "\x01" "dynq" + std::to_string(ni) + "." + std::to_string(k) : nd.out[k];
    if (!(p.y = make_q_out(names[0], shape, DT_UINT8))) return false;
    if (!(p.scale = make_out(names[1], {}))) return false;
    if (!(p.zp = make_q_out(names[2], {}, DT_UINT8))) return false;
    if (!dalloc(&p.part, (size_t)kDynParts * 2 * sizeof(float))) return false;
    p.blocks = dyn_blocks(p.n);
    emit("vso::k_dyn_minmax(vso::DynQParams)", p, launch_dyn_minmax);
    emit("vso::k_dyn_quantize(vso::DynQParams)", p, launch_dyn_quantize);
    return q_publish(names[0]) && q_publish(names[2]);
  }

  struct DynFuse {
    int cast, mul, smul;  // Cast, Mul(., s), s = Mul(x_scale, w_scale)
    int add, act;         // Add(constant bias), Relu / Clip (-1: none)
  };
  std::map<size_t, DynFuse> dynfuse;  // by ConvInteger / MatMulInteger node (find_dynq)

  // a value the walk will know as a constant: an initializer, or computed from such alone
  bool const_deep(const std::string& n, int depth = 0) {
    if (n.empty() || depth > 8) return false;
    if (Value* v = val(n)) return v->is_const;
    const int p = producer(n);
    if (p < 0) return false;
    const Node& nd = g.nodes[p];
    if (nd.op == "Constant") return true;
    if (nd.in.empty()) return false;
    for (const std::string& i : nd.in)
      if (!i.empty() && !const_deep(i, depth + 1)) return false;
    return true;
  }
  static const std::string& other_operand(const Node& nd, const std::string& name) {
    return nd.in[0] == name ? nd.in[1] : nd.in[0];
  }

  void find_dynq() {
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      const Node& nd = g.nodes[k];
      if ((nd.op != "ConvInteger" && nd.op != "MatMulInteger") || done.count(k) || nd.out.empty() || nd.in.size() < 2) continue;
      DynFuse f{-1, -1, -1, -1, -1};
      f.cast = sole_consumer(nd.out[0], k);
      if (f.cast < 0 || g.nodes[f.cast].op != "Cast" || g.nodes[f.cast].ai("to", DT_FLOAT) != DT_FLOAT || done.count((size_t)f.cast))
        continue;
      const std::string& fl = g.nodes[f.cast].out[0];
      f.mul = sole_consumer(fl, (size_t)f.cast);
      if (f.mul < 0 || g.nodes[f.mul].op != "Mul" || g.nodes[f.mul].in.size() != 2 || done.count((size_t)f.mul)) continue;
      const std::string& sname = other_operand(g.nodes[f.mul], fl);
      f.smul = producer(sname);
      if (sname == fl || f.smul < 0 || g.nodes[f.smul].op != "Mul" || g.nodes[f.smul].in.size() != 2 ||
          done.count((size_t)f.smul) || consumers[sname] != 1 || is_graph_output(sname))
        continue;
      // x_scale: output 1 of the DynamicQuantizeLinear that made input 0; w_scale: a constant
      const int pd = producer(nd.in[0]);
      if (pd < 0 || g.nodes[pd].op != "DynamicQuantizeLinear" || g.nodes[pd].out.size() < 2 || g.nodes[pd].out[1].empty()) continue;
      const std::string& xs = g.nodes[pd].out[1];
      const Node& sm = g.nodes[f.smul];
      if ((sm.in[0] == xs) == (sm.in[1] == xs) || !const_deep(other_operand(sm, xs))) continue;
      std::string out = g.nodes[f.mul].out[0];
      size_t last = (size_t)f.mul;
      int c = sole_consumer(out, last);
      if (c >= 0 && g.nodes[c].op == "Add" && g.nodes[c].in.size() == 2 && !done.count((size_t)c)) {
        const std::string& b = other_operand(g.nodes[c], out);
        if (b == out || !const_deep(b)) continue;  // (a runtime bias: the nodes as they are)
        f.add = c;
        out = g.nodes[c].out[0];
        last = (size_t)c;
        c = sole_consumer(out, last);
      }
      if (c >= 0 && (g.nodes[c].op == "Relu" || g.nodes[c].op == "Clip") && g.nodes[c].in[0] == out && !done.count((size_t)c)) {
        bool ok = true;
        for (size_t q = 1; q < g.nodes[c].in.size(); ++q) ok = ok && (g.nodes[c].in[q].empty() || const_deep(g.nodes[c].in[q]));
        if (ok) f.act = c;
      }
      for (int q : {f.cast, f.mul, f.smul, f.add, f.act})
        if (q >= 0) done.insert((size_t)q);
      dynfuse[k] = f;
    }
  }

  // a constant of one value, or of `channels` values lying along the channel axis of a rank-`rank` output
  // (`axis` from the left: 1 of a ConvInteger's NCHW, the last of a MatMulInteger's) under ONNX broadcasting
  static bool channel_const(const Value* v, int64_t channels, size_t rank, size_t axis, bool one_ok) {
    if (!v || !v->is_const || v->c.is_int || v->c.f16 || v->c.f.empty()) return false;
    const std::vector<int64_t>& d = v->c.dims;
    if (d.size() > rank) return false;
    const int64_t n = v->c.numel();
    if (n == 1) return one_ok || channels == 1;
    if (n != channels) return false;
    for (size_t q = 0; q < d.size(); ++q)
      if (d[q] != 1 && q + rank - d.size() != axis) return false;
    return true;
  }

  struct Fused {  // the float epilogue of a fused chain
    const float* xscale = nullptr;
    std::vector<float> wscale, bias;
    int act = ACT_NONE;
    float lo = 0.f, hi = 0.f;
    std::string out;
  };

  // the node heading a chain of find_dynq: 1 planned as one launch, 0 left to the nodes as they are, -1 failed
  int try_plan_dynq(size_t ni) {
    const DynFuse f = dynfuse[ni];
    dynfuse.erase(ni);
    const Node& nd = g.nodes[ni];
    auto unfuse = [&]() -> int {
      for (int q : {f.cast, f.mul, f.smul, f.add, f.act})
        if (q >= 0) done.erase((size_t)q);
      // (the scalar Mul placed ahead of this node: its launch now; behind it: when the walk reaches it)
      return (size_t)f.smul < ni && !plan_node((size_t)f.smul) ? -1 : 0;
    };
    const bool mm = nd.op == "MatMulInteger";
    Value* x = val(nd.in[0]);
    Value* w = val(nd.in[1]);
    if (!x || !w || !w->is_const || w->c.dims.size() != (mm ? 2u : 4u) || x->shape.size() < 2) return unfuse();  // (refused below, by name)
    const int64_t M = mm ? w->c.dims[1] : w->c.dims[0];
    const size_t rank = x->shape.size(), axis = mm ? rank - 1 : 1;
    const Node& sm = g.nodes[f.smul];
    const int pd = producer(nd.in[0]);
    const std::string& xsn = g.nodes[pd].out[1];
    Value* xs = val(xsn);
    Value* ws = val(other_operand(sm, xsn));
    if (!xs || xs->is_const || xs->qtype || xs->numel() != 1 || !channel_const(ws, M, rank, axis, true)) return unfuse();
    Fused fu{};
    fu.xscale = dptr(*xs);
    fu.wscale.assign((size_t)M, 0.f);
    for (int64_t m = 0; m < M; ++m) fu.wscale[m] = ws->c.f[ws->c.numel() == 1 ? 0 : m];
    fu.out = g.nodes[f.mul].out[0];
    if (f.add >= 0) {
      Value* b = val(other_operand(g.nodes[f.add], fu.out));
      if (!channel_const(b, M, rank, axis, false)) return unfuse();
      fu.bias = b->c.f;
      fu.out = g.nodes[f.add].out[0];
    }
    if (f.act >= 0) {
      Epilogue ep{};
      if (!act_of(g.nodes[f.act], &ep, (int)M)) return unfuse();
      fu.act = ep.act; fu.lo = ep.a0; fu.hi = ep.a1;
      fu.out = g.nodes[f.act].out[0];
    }
    return emit_integer(nd, &fu) ? 1 : -1;
  }

  bool plan_integer(size_t, const Node& nd, Ins&) { return emit_integer(nd, nullptr); }

  // ConvInteger / MatMulInteger (the 1x1 convolution of N = rows, C = K, H = W = 1): k_iconv_tile where group is
  // 1 and K < 2^15, else k_iconv_direct; fu: with the float epilogue, written as the chain's output
  bool emit_integer(const Node& nd, const Fused* fu) {
    const bool mm = nd.op == "MatMulInteger";
    const std::string at = nd.op + " '" + nd.name + "': unsupported: ";
    Value* in[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t k = 0; k < 4 && k < nd.in.size(); ++k)
      if (!nd.in[k].empty() && !(in[k] = val(nd.in[k])))
        return fail("node '" + nd.name + "' (" + nd.op + "): input '" + nd.in[k] + "' is not defined");
    Value *x = in[0], *w = in[1], *zx = in[2], *zw = in[3];
    if (!x || x->is_const || (x->qtype != DT_UINT8 && x->qtype != DT_INT8))
      return fail(at + "input 0 must be a quantised runtime tensor (uint8 / int8: DynamicQuantizeLinear, QuantizeLinear)");
    if (!w || !w->is_const) return fail(at + "the weights (input 1) must be a constant");
    if (!w->c.is_int || (w->c.dtype != DT_UINT8 && w->c.dtype != DT_INT8)) return fail(at + "uint8 / int8 weights only");
    if (zw && !zw->is_const) return fail(at + "the weights' zero point (input 3) must be a constant");
    if (zx && (zx->numel() != 1 || (zx->is_const ? !zx->c.is_int || zx->c.dtype != x->qtype : zx->qtype != x->qtype)))
      return fail(at + "the input's zero point (input 2) must be one value of the input's type");
    IConvParams p{};
    std::vector<int64_t> oshape;
    if (mm) {
      const std::vector<int64_t>& as_ = x->shape;
      if (w->c.dims.size() != 2) return fail(at + "a constant B of rank 2 only");
      if (as_.size() < 2) return fail(at + "an A of rank >= 2 only");
      if (as_.back() != w->c.dims[0]) return fail(nd.op + " '" + nd.name + "': inner dimensions differ");
      p.C = (int)as_.back();
      p.N = (int)(x->numel() / std::max<int64_t>(p.C, 1));
      p.M = (int)w->c.dims[1];
      p.H = p.W = p.Ho = p.Wo = p.kh = p.kw = p.sh = p.sw = p.dh = p.dw = p.G = 1;
      p.Cg = p.C;
      p.Mg = p.M;
      oshape.assign(as_.begin(), as_.end() - 1);
      oshape.push_back(p.M);
    } else {
      Node geo = nd;  // (inputs 2 and 3 are zero points, no bias: the attributes, list lengths and refusals are Conv's)
      geo.in.resize(2);
      ConvPlan c;
      if (!conv_geometry(geo, &c)) return false;
      const ConvParams& cp = c.p;
      p.N = cp.N; p.C = cp.C; p.H = cp.H; p.W = cp.W; p.M = cp.M; p.Ho = cp.Ho; p.Wo = cp.Wo;
      p.G = cp.G; p.Cg = cp.Cg; p.Mg = cp.Mg;
      p.kh = cp.kh; p.kw = cp.kw; p.sh = cp.sh; p.sw = cp.sw; p.dh = cp.dh; p.dw = cp.dw; p.pt = cp.pt; p.pl = cp.pl;
      oshape = c.oshape;
    }
    const int64_t K64 = (int64_t)p.Cg * p.kh * p.kw;
    if (p.M < 1 || K64 < 1 || K64 >= (int64_t{1} << 30) || (int64_t)p.N * p.M * p.Ho * p.Wo >= (int64_t{1} << 30))
      return fail(at + "2^30 elements or more");
    p.K = (int)K64;
    const int64_t nz = zw ? zw->c.numel() : 1;
    if (zw && (!zw->c.is_int || zw->c.dtype != w->c.dtype || (nz != 1 && nz != p.M)))
      return fail(at + "the weights' zero point (input 3) must be one value or one per output channel, of the weights' type");
    // signed bytes: w' = Wq - 128 with zw' = zw - 128 (uint8), or as they are (int8)
    const int off = w->c.dtype == DT_UINT8 ? 128 : 0;
    std::vector<signed char> wi((size_t)p.M * p.K);
    std::vector<int> wsum((size_t)p.M, 0), zwv((size_t)p.M, 0);
    bool any_zw = false;
    for (int m = 0; m < p.M; ++m) {
      zwv[m] = (int)(zw ? zw->c.i[nz == 1 ? 0 : m] : 0) - off;
      any_zw = any_zw || zwv[m] != 0;
      for (int k = 0; k < p.K; ++k) {
        const int64_t v = (mm ? w->c.i[(size_t)k * p.M + m] : w->c.i[(size_t)m * p.K + k]) - off;
        wi[(size_t)m * p.K + k] = (signed char)v;
        wsum[m] += (int)v;
      }
    }
    const bool tile = p.G == 1 && p.K < (1 << 15);
    if (tile) {
      p.Kp = (p.K + kQK - 1) / kQK * kQK;
      p.Mp = (p.M + kQBM - 1) / kQBM * kQBM;
      std::vector<signed char> packed((size_t)p.Mp * p.Kp, 0);
      for (int m = 0; m < p.M; ++m) std::copy(wi.begin() + (size_t)m * p.K, wi.begin() + (size_t)(m + 1) * p.K, packed.begin() + (size_t)m * p.Kp);
      if (!(p.w = static_cast<const signed char*>(upload_bytes(packed.data(), packed.size())))) return false;
      if (!(p.wsum = static_cast<const int*>(upload_bytes(wsum.data(), wsum.size() * 4)))) return false;
      p.rows = p.H == 1 && p.W == 1 && p.kh == 1 && p.kw == 1 && p.pt == 0 && p.pl == 0;
    } else if (!(p.w = static_cast<const signed char*>(upload_bytes(wi.data(), wi.size())))) {
      return false;
    }
    if (any_zw && !(p.zw = static_cast<const int*>(upload_bytes(zwv.data(), zwv.size() * 4)))) return false;
    p.xflip = x->qtype == DT_UINT8 ? 0x80 : 0;
    if (zx && zx->is_const) {
      const unsigned char b = (unsigned char)(int)zx->c.i[0];
      if (!(p.zx = static_cast<const unsigned char*>(upload_bytes(&b, 1)))) return false;
    } else if (zx) {
      p.zx = qptr(*zx);
    }
    p.x = qptr(*x);
    if (fu) {
      p.xscale = fu->xscale;
      if (!(p.wscale = upload_vec(fu->wscale))) return false;
      if (!fu->bias.empty() && !(p.bias = upload_vec(fu->bias))) return false;
      p.act = fu->act; p.lo = fu->lo; p.hi = fu->hi;
      if (!(p.yf = make_out(fu->out, oshape))) return false;
      s->dynq_nodes++;
    } else if (!(p.yi = reinterpret_cast<int*>(make_q_out(nd.out[0], oshape, DT_INT32)))) {
      return false;
    }
    if (tile) emit("vso::k_iconv_tile(vso::IConvParams)", p, launch_iconv_tile);
    else emit("vso::k_iconv_direct(vso::IConvParams)", p, launch_iconv_direct);
    return true;
  }

  // ---- the walk ------------------------------------------------------------
  static std::vector<Operand> operands(const Ins& in) {
    std::vector<Operand> o;
    for (const Value* v : in) o.push_back(v ? Operand{&v->shape, v->is_const ? &v->c : nullptr} : Operand{});
    return o;
  }

  using PlanOp = bool (Planner::*)(size_t, const Node&, Ins&);
  static PlanOp plan_of(const std::string& op) {
    static const std::map<std::string, PlanOp> ops = {
        {"Conv", &Planner::plan_conv},
        {"Reshape", &Planner::plan_view}, {"Flatten", &Planner::plan_view},
        {"Squeeze", &Planner::plan_view}, {"Unsqueeze", &Planner::plan_view},
        {"Identity", &Planner::plan_alias}, {"Dropout", &Planner::plan_alias}, {"Cast", &Planner::plan_cast},
        {"Relu", &Planner::plan_activation}, {"Clip", &Planner::plan_activation},
        {"PRelu", &Planner::plan_activation}, {"LeakyRelu", &Planner::plan_activation},
        {"Sigmoid", &Planner::plan_activation}, {"Tanh", &Planner::plan_activation},
        {"HardSigmoid", &Planner::plan_activation}, {"HardSwish", &Planner::plan_activation},
        {"Gelu", &Planner::plan_activation}, {"Erf", &Planner::plan_activation},
        {"LayerNormalization", &Planner::plan_layer_norm},
        {"ConvTranspose", &Planner::plan_conv_transpose}, {"ReduceMean", &Planner::plan_reduce_mean},
        {"Add", &Planner::plan_arith}, {"Sub", &Planner::plan_arith},
        {"Mul", &Planner::plan_arith}, {"Div", &Planner::plan_arith},
        {"MaxPool", &Planner::plan_pool}, {"AveragePool", &Planner::plan_pool},
        {"GlobalAveragePool", &Planner::plan_global_pool},
        {"InstanceNormalization", &Planner::plan_instance_norm},
        {"BatchNormalization", &Planner::plan_batch_norm},
        {"Softmax", &Planner::plan_softmax}, {"LogSoftmax", &Planner::plan_log_softmax},
        {"ArgMax", &Planner::plan_argmax}, {"ReduceMax", &Planner::plan_reduce_max}, {"Gather", &Planner::plan_gather},
        {"Transpose", &Planner::plan_transpose}, {"Pad", &Planner::plan_pad},
        {"Concat", &Planner::plan_concat}, {"Split", &Planner::plan_split}, {"Slice", &Planner::plan_slice},
        {"Resize", &Planner::plan_resize}, {"Upsample", &Planner::plan_resize},
        {"Gemm", &Planner::plan_gemm}, {"MatMul", &Planner::plan_matmul},
        {"MatMulNBits", &Planner::plan_matmul_nbits},
        {"QuantizeLinear", &Planner::plan_quantize}, {"DequantizeLinear", &Planner::plan_dequantize},
        {"DynamicQuantizeLinear", &Planner::plan_dynamic_quantize},
        {"ConvInteger", &Planner::plan_integer}, {"MatMulInteger", &Planner::plan_integer}};
    auto it = ops.find(op);
    return it == ops.end() ? nullptr : it->second;
  }

  // input resolution, then: a constant node is folded on the host, a runtime
  // node goes to its operator's plan
  bool plan_node(size_t ni) {
    if (attn.count(ni)) {  // the second MatMul of an attention pattern: one k_attn launch, or the nodes as they are
      const int r = try_plan_attn(ni);
      if (r != 0) return r > 0;
    }
    if (qfuse.count(ni)) {  // the Conv / Add of a quantised pattern: one launch on the integers, or the nodes as they are
      const int r = try_plan_q(ni);
      if (r != 0) return r > 0;
    }
    if (dynfuse.count(ni)) {  // a ConvInteger / MatMulInteger heading a chain: one launch with the float epilogue, or the nodes as they are
      const int r = try_plan_dynq(ni);
      if (r != 0) return r > 0;
    }
    const Node& nd = g.nodes[ni];
    const std::string& op = nd.op;
    Ins in;
    bool all_const = true;
    for (const std::string& n : nd.in) {
      if (n.empty()) { in.push_back(nullptr); continue; }
      Value* v = val(n);
      if (!v) return fail("node '" + nd.name + "' (" + op + "): input '" + n + "' is not defined");
      in.push_back(v);
      all_const = all_const && v->is_const;
    }
    // a 16-bit integer or float8 constant (read as its type alone): Quantize / DequantizeLinear of a runtime
    // tensor say so themselves (q_params), nothing else reads one
    for (const Value* v : in)
      if (v && v->is_const && opaque_type(v->c.dtype) &&
          !((op == "QuantizeLinear" || op == "DequantizeLinear") && in[0] && !in[0]->is_const))
        return fail(op + " '" + nd.name + "': unsupported: a constant of type " + std::to_string(v->c.dtype) +
                    " (16-bit integer and float8 tensors are not computed on)");
    if (op != "Conv" && op != "Concat")
      for (const std::string& n : nd.in) flush_up(n);
    if (!is_head_op(op))
      for (const std::string& n : nd.in)
        if (!flush_head(n)) return false;
    if (op == "Shape" || (all_const && !in.empty() && op != "Conv") || op == "Constant") {
      Const r;
      if (!fold(nd, operands(in), &r, &err)) return false;
      set_const(nd.out[0], r);
      return true;
    }
    const PlanOp plan = plan_of(op);
    if (!plan) return fail("unsupported operator " + op + " (node '" + nd.name + "')");
    // (a quantised tensor's buffer is a quarter of the floats, an int32 one holds integers: no float kernel may read either)
    const bool integer = op == "ConvInteger" || op == "MatMulInteger";
    for (size_t k = 0; k < in.size(); ++k) {
      const Value* v = in[k];
      if (!v || !v->qtype) continue;
      if (v->qtype == DT_INT32 ? !(op == "Cast" && k == 0) : !((op == "DequantizeLinear" && k == 0) || (integer && (k == 0 || k == 2))))
        return fail(op + " '" + nd.name + "': unsupported: " +
                    (v->qtype == DT_INT32 ? "an int32 tensor is read by Cast to FLOAT only"
                                          : "a quantised tensor is read by DequantizeLinear, ConvInteger and MatMulInteger only"));
    }
    return (this->*plan)(ni, nd, in);
  }

  bool run(const std::vector<std::vector<int64_t>>& in_shapes) {
    for (const Node& nd : g.nodes)
      for (const std::string& i : nd.in)
        if (!i.empty()) consumers[i]++;
    for (auto& kv : g.inits) set_const(kv.first, kv.second);
    for (size_t k = 0; k < g.inputs.size(); ++k) {
      if (!set_runtime(g.inputs[k].name, in_shapes[k])) return false;
      s->in_names.push_back(g.inputs[k].name);
      s->in_shapes.push_back(in_shapes[k]);
      s->in_bufs.push_back(vals[g.inputs[k].name].buf);
    }
    if (!check_quantised_readers()) return false;
    find_hswish();
    find_gelu();
    if (attn_enabled()) find_attention();
    find_residual_fusions();
    find_ibnorm();
    find_concat_direct();
    if (s->conv_precision != PREC_F32) find_up_fusions();
    if (head_enabled()) find_heads();
    if (qdq_enabled()) find_qdq();
    if (dynq_enabled()) find_dynq();
    for (size_t k = 0; k < g.nodes.size(); ++k) {
      if (done.count(k)) continue;
      if (!plan_node(k)) return false;
    }
    if (!up_pending.empty()) return fail("internal: Resize '" + up_pending.begin()->first + "' never launched");
    if (!head_pending.empty()) return fail("internal: Resize '" + head_pending.begin()->first + "' never computed");
    if (!cat_tail.empty()) return fail("internal: Concat input copy into '" + cat_tail.begin()->first + "' never launched");
    if (!norm_pending.empty()) return fail("internal: InstanceNorm of '" + norm_pending.begin()->first + "' never applied");
    if (!pending_dw.empty()) return fail("internal: depthwise Conv into '" + pending_dw.begin()->first + "' never computed");
    for (const IO& o : g.outputs) {
      Value* v = val(o.name);
      if (!v) return fail("graph output '" + o.name + "' is never produced");
      if (v->is_const) {  // a constant output: materialise it once
        const float* d = upload(v->c);
        if (!d) return false;
        const int b = new_buf(v->c.numel());
        if (b < 0) return false;
        if (hipMemcpy(s->bufs[b], d, v->c.numel() * 4, hipMemcpyDeviceToDevice) != hipSuccess)
          return fail("constant output copy failed");
        v->buf = b;
      }
      s->out_names.push_back(o.name);
      s->out_shapes.push_back(v->shape);
      // (a quantised output: its type whatever the model declares, the buffer q_publish filled)
      s->out_types.push_back(v->qtype ? v->qtype : o.elem_type ? o.elem_type : (int)DT_FLOAT);
      s->out_bufs.push_back(v->qtype ? q_out.at(o.name) : v->buf);
    }
    return true;
  }
};

}  // namespace

bool plan_session(vso_session* s, Graph& g, const std::vector<std::vector<int64_t>>& in_shapes, std::string* err) {
  Planner pl{s, g};
  const bool ok = pl.run(in_shapes);
  *err = pl.err;
  return ok;
}
