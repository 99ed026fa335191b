// vso_session.h — what the planner (vso_plan.hip) builds and the runtime
// (vso_model.hip) runs: a session's tensors, device allocations and launch
// list; and the helpers that read the A/B knobs from the environment.
// Internal to libvss.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "vso_onnx.h"

// A graph value while planning: a constant, or a runtime tensor in a device buffer.
struct Value {
  std::vector<int64_t> shape;
  bool is_const = false;
  vso_onnx::Const c;  // when is_const
  int buf = -1;       // runtime tensor: device buffer id
  int qtype = 0;      // runtime tensor: 0 float32, or DT_UINT8 / DT_INT8: quantised, one byte per element in `buf`,
                      // or DT_INT32 (a ConvInteger / MatMulInteger output): four bytes per element
  int64_t numel() const {
    int64_t n = 1;
    for (int64_t d : shape) n *= d;
    return n;
  }
};

// A host region holding a launch's parameters: at capture, every aligned
// 8-byte word of it that points into one of the session's device
// allocations marks that allocation as used by the launch (read or written:
// the lane schedule treats every use as a conflict).
struct Region {
  std::shared_ptr<const void> keep;
  const void* p;
  size_t n;
};

struct Launch {
  std::string name;
  std::function<void(hipStream_t)> fn;
  std::vector<Region> io;
};

struct DevRange {
  uintptr_t lo, hi;
  bool ro;  // constants: never written by a kernel (no dependency through them)
};

struct vso_session {
  int device = 0;
  int conv_precision = 0;  // ConvPrec
  int tile_convs = 0;      // convolutions planned on k_conv_tile
  int ir_blocks = 0;       // inverted residual blocks planned on k_ir
  int attn_nodes = 0;      // attention patterns planned on k_attn (vso_attn_count)
  int head_nodes = 0;      // fused class heads planned on k_class_head (vso_head_count)
  int qconv_nodes = 0;     // fused quantised launches: k_qconv_tile + k_qconv_dw + k_qadd (vso_qconv_count)
  int dynq_nodes = 0;      // ConvInteger / MatMulInteger chains planned as one launch with the float epilogue (vso_dynq_count)
  hipStream_t stream = nullptr;
  std::string err;
  std::vector<std::string> in_names, out_names;
  std::vector<std::vector<int64_t>> in_shapes, out_shapes;
  std::vector<int> out_types;  // each output's declared ONNX element type (vso_output_type; the buffers are f32)
  std::vector<float*> bufs;
  std::vector<int64_t> buf_elems;
  std::vector<int> in_bufs, out_bufs;
  std::vector<void*> allocs;
  std::vector<Launch> launches;
  std::vector<DevRange> ranges;   // every device allocation of the session
  hipStream_t side = nullptr;     // the second capture lane
  std::vector<hipEvent_t> events; // cross-lane edges of the captured graph
  int lanes_used = 1;             // lanes of the captured schedule (vso_lane_count)
  hipGraphExec_t graph = nullptr;
  std::atomic<int> busy{0};
};

// Plans `g` with the given input shapes into s->launches (allocating and
// uploading on s->device); false with *err set.
__attribute__((visibility("hidden"))) bool plan_session(vso_session* s, vso_onnx::Graph& g,
                                                        const std::vector<std::vector<int64_t>>& in_shapes,
                                                        std::string* err);

// The A/B knobs (VSO_*): read through a `static const` local at the call
// site, so once per process.  env_on: on unless set to 0; env_off: off unless
// set to 1; env_int: the value, or `dflt` when unset.
static inline bool env_on(const char* n) { const char* e = std::getenv(n); return !(e && e[0] == '0'); }
static inline bool env_off(const char* n) { const char* e = std::getenv(n); return e && e[0] == '1'; }
static inline long env_int(const char* n, long dflt) { const char* e = std::getenv(n); return e ? std::atol(e) : dflt; }
