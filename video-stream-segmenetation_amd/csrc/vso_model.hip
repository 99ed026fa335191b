// vso_model.hip — ONNX sessions (include/vso.h): the C ABI and the run time.
// vso_create reads the model (vso_onnx.cpp) and plans it into a fixed launch
// list over preallocated HBM tensors (vso_plan.hip); a run captures that list
// once in a hipGraph, on one or two lanes, and replays it.
//
// What it replaces: onnxruntime-web's InferenceSession as the reference uses
// it (client/src/core/model.ts:12-67; session.run at frameProcessorTest.ts:91,
// :406, :478), through the same kind of entry points as ORT-web's wasm
// exports (_OrtCreateSession / _OrtRun / _OrtGetLastError,
// client/public/ort-wasm-simd-threaded.mjs:50-53).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/vso.h"
#include "vso_session.h"

namespace {

thread_local std::string g_err;

int fail_s(vso_session* s, int code, const std::string& m) {
  if (s) s->err = m;
  else g_err = m;
  return code;
}

int64_t numel(const std::vector<int64_t>& v) {
  int64_t n = 1;
  for (int64_t d : v) n *= d;
  return n;
}

// Two capture lanes (VSO_LANES=1: one).  Launch i uses the device allocations
// its parameter regions point into (constants excepted); it depends on the
// last earlier launch that used each of them (every use counts as a write, so
// the users of an allocation form one chain).  List scheduling in launch
// order, unit costs: a launch starts on the lane where it can start first
// (ties: the lane of its latest dependency, then lane 0); a dependency on the
// other lane becomes an event edge.  MODNet: the HR branch's entry (the
// image resizes, e2 / e4, the first HR convolutions) runs on lane 1 beside
// the backbone's latency-bound blocks (tools/micro/graph_branches.hip:
// independent branches of one captured graph run concurrently).
struct LaneSchedule {
  std::vector<int> lane, wait_on;  // wait_on: the other lane's launch to wait for, or -1
  std::vector<char> record;        // an event is recorded after this launch
  int used = 1;
};

LaneSchedule schedule_lanes(const vso_session* s, int lanes) {
  const size_t n = s->launches.size();
  LaneSchedule ls;
  ls.lane.assign(n, 0);
  ls.wait_on.assign(n, -1);
  ls.record.assign(n, 0);
  if (lanes < 2 || n < 2) return ls;
  std::vector<DevRange> rs = s->ranges;
  std::sort(rs.begin(), rs.end(), [](const DevRange& a, const DevRange& b) { return a.lo < b.lo; });
  auto find = [&](uintptr_t v) -> int {
    size_t lo = 0, hi = rs.size();
    while (lo < hi) {  // the last range with lo <= v
      const size_t mid = (lo + hi) / 2;
      if (rs[mid].lo <= v) lo = mid + 1;
      else hi = mid;
    }
    if (lo == 0) return -1;
    const DevRange& r = rs[lo - 1];
    return v < r.hi && !r.ro ? (int)(lo - 1) : -1;
  };
  std::vector<int> last(rs.size(), -1), fin(n, 0);
  int ready_at[2] = {0, 0};
  for (size_t i = 0; i < n; ++i) {
    std::set<int> deps;
    std::set<int> used;
    // a launch that registered no parameter block: unknown buffers, so it
    // conflicts with every buffer (ordered after and before everything)
    if (s->launches[i].io.empty())
      for (int k = 0; k < (int)rs.size(); ++k) used.insert(k);
    for (const Region& rg : s->launches[i].io)
      for (size_t o = 0; o + 8 <= rg.n; o += 8) {
        uint64_t v;
        std::memcpy(&v, static_cast<const char*>(rg.p) + o, 8);
        const int k = find((uintptr_t)v);
        if (k >= 0) used.insert(k);
      }
    for (int k : used)
      if (last[k] >= 0) deps.insert(last[k]);
    int ready = 0, latest = -1;
    for (int d : deps) {
      ready = std::max(ready, fin[d]);
      if (latest < 0 || fin[d] > fin[latest]) latest = d;
    }
    int best = 0, best_start = std::max(ready, ready_at[0]);
    const int s1 = std::max(ready, ready_at[1]);
    if (s1 < best_start || (s1 == best_start && latest >= 0 && ls.lane[latest] == 1)) {
      best = 1;
      best_start = s1;
    }
    ls.lane[i] = best;
    fin[i] = best_start + 1;
    ready_at[best] = fin[i];
    int w = -1;
    for (int d : deps)
      if (ls.lane[d] != best) w = std::max(w, d);
    if (w >= 0) {
      ls.wait_on[i] = w;
      ls.record[w] = 1;
    }
    for (int k : used) last[k] = (int)i;
    if (best == 1) ls.used = 2;
  }
  return ls;
}

// Two lanes for sessions of >= 2^21 input elements (MODNet batch 8 at
// 288x512: 1.41 -> 1.35 ms bf16, 3.88 -> 3.72 f32), one below: at batch 1 and
// on the MediaPipe nets the cross-lane edges cost more than the overlap gives
// (MODNet batch 1 0.594 -> 0.62 ms, the face detector 0.405 -> 0.447 ms;
// profiles/r05u).  VSO_LANES=1 / 2 forces either.
int lanes_wanted(const vso_session* s) {
  static const int forced =
      std::getenv("VSO_LANES") ? std::max(1, std::min(2, (int)env_int("VSO_LANES", 0))) : 0;
  if (forced) return forced;
  return !s->in_shapes.empty() && numel(s->in_shapes[0]) >= (int64_t{1} << 21) ? 2 : 1;
}

int run_graph(vso_session* s, hipStream_t st) {
  if (!s->graph) {  // capture the launch list once (buffers are the session's own)
    hipGraph_t g = nullptr;
    hipStream_t cs = s->stream;
    const LaneSchedule ls = schedule_lanes(s, lanes_wanted(s));
    if (ls.used > 1 && !s->side && hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking) != hipSuccess)
      return fail_s(s, VSO_E_HIP, "hipStreamCreate failed");
    const size_t n = s->launches.size();
    std::vector<hipEvent_t> ev(n, nullptr);
    hipEvent_t fork = nullptr, join = nullptr;
    if (ls.used > 1) {
      for (size_t i = 0; i < n; ++i)
        if (ls.record[i]) {
          if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess)
            return fail_s(s, VSO_E_HIP, "hipEventCreate failed");
          s->events.push_back(ev[i]);
        }
      if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&join, hipEventDisableTiming) != hipSuccess)
        return fail_s(s, VSO_E_HIP, "hipEventCreate failed");
      s->events.push_back(fork);
      s->events.push_back(join);
    }
    if (hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed) != hipSuccess)
      return fail_s(s, VSO_E_HIP, "hipStreamBeginCapture failed");
    bool ok = true;
    if (ls.used > 1)  // the side lane joins the capture
      ok = hipEventRecord(fork, cs) == hipSuccess && hipStreamWaitEvent(s->side, fork, 0) == hipSuccess;
    for (size_t i = 0; i < n && ok; ++i) {
      hipStream_t ls_st = ls.lane[i] ? s->side : cs;
      if (ls.wait_on[i] >= 0) ok = hipStreamWaitEvent(ls_st, ev[ls.wait_on[i]], 0) == hipSuccess;
      if (!ok) break;  // (never captured without its cross-lane dependency)
      s->launches[i].fn(ls_st);
      if (ls.record[i]) ok = hipEventRecord(ev[i], ls_st) == hipSuccess;
    }
    if (ls.used > 1) {  // the side lane rejoins the capture, also after a failure (so it can end)
      const bool joined = hipEventRecord(join, s->side) == hipSuccess && hipStreamWaitEvent(cs, join, 0) == hipSuccess;
      ok = ok && joined;
    }
    const hipError_t e = hipStreamEndCapture(cs, &g);
    if (!ok) {
      if (g) (void)hipGraphDestroy(g);
      if (s->side) {  // whatever capture state it was left in: a fresh side stream next time
        (void)hipStreamDestroy(s->side);
        s->side = nullptr;
      }
      return fail_s(s, VSO_E_HIP, "capturing the lane schedule failed");
    }
    s->lanes_used = ls.used;
    if (e != hipSuccess || !g) return fail_s(s, VSO_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    const hipError_t e2 = hipGraphInstantiate(&s->graph, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e2 != hipSuccess) return fail_s(s, VSO_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e2));
  }
  if (hipGraphLaunch(s->graph, st) != hipSuccess) return fail_s(s, VSO_E_HIP, "hipGraphLaunch failed");
  return VSO_OK;
}

struct Busy {
  vso_session* s;
  bool ok;
  explicit Busy(vso_session* ss) : s(ss) {
    int z = 0;
    ok = s->busy.compare_exchange_strong(z, 1);
  }
  ~Busy() { if (ok) s->busy.store(0); }
};

}  // namespace

extern "C" {

void vso_options_default(vso_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->conv_precision = VSO_PRECISION_F32;
}

int vso_create(const void* model, size_t bytes, const int64_t* input_dims, int input_ndim, int device_id,
               vso_session** out) {
  return vso_create_ex(model, bytes, input_dims, input_ndim, device_id, nullptr, out);
}

int vso_create_ex(const void* model, size_t bytes, const int64_t* input_dims, int input_ndim, int device_id,
                  const vso_options* opts, vso_session** out) {
  if (!model || !bytes || !out) return fail_s(nullptr, VSO_E_INVALID_ARG, "null model/out");
  vso_options o;
  vso_options_default(&o);
  if (opts) o = *opts;
  if (o.conv_precision < VSO_PRECISION_F32 || o.conv_precision > VSO_PRECISION_F16)
    return fail_s(nullptr, VSO_E_INVALID_ARG, "conv_precision must be VSO_PRECISION_F32, _BF16 or _F16");
  *out = nullptr;
  vso_onnx::Graph g;
  std::string err;
  if (!vso_onnx::parse_model(static_cast<const uint8_t*>(model), bytes, &g, &err))
    return fail_s(nullptr, VSO_E_PARSE, err);
  if (g.inputs.empty()) return fail_s(nullptr, VSO_E_UNSUPPORTED, "model has no runtime inputs");
  std::vector<std::vector<int64_t>> shapes;
  for (size_t k = 0; k < g.inputs.size(); ++k) {
    std::vector<int64_t> d = g.inputs[k].dims;
    if (k == 0 && input_dims && input_ndim > 0) d.assign(input_dims, input_dims + input_ndim);
    for (int64_t v : d)
      if (v < 1) return fail_s(nullptr, VSO_E_INVALID_ARG, "input '" + g.inputs[k].name + "' has symbolic dims: pass input_dims");
    shapes.push_back(d);
  }
  vso_session* s = new vso_session();
  s->device = device_id;
  s->conv_precision = o.conv_precision;
  if (hipSetDevice(device_id) != hipSuccess) {
    delete s;
    return fail_s(nullptr, VSO_E_HIP, "hipSetDevice failed");
  }
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
    delete s;
    return fail_s(nullptr, VSO_E_HIP, "hipStreamCreate failed");
  }
  if (!plan_session(s, g, shapes, &err)) {
    const bool unsup = err.find("unsupported") != std::string::npos || err.find("only") != std::string::npos;
    vso_destroy(s);
    return fail_s(nullptr, unsup ? VSO_E_UNSUPPORTED : VSO_E_INVALID_ARG, err);
  }
  *out = s;
  return VSO_OK;
}

void vso_destroy(vso_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->graph) (void)hipGraphExecDestroy(s->graph);
  for (hipEvent_t e : s->events) (void)hipEventDestroy(e);
  for (void* p : s->allocs) (void)hipFree(p);
  if (s->side) (void)hipStreamDestroy(s->side);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

const char* vso_last_error(const vso_session* s) { return s ? s->err.c_str() : g_err.c_str(); }

int vso_io_count(const vso_session* s, int* n_in, int* n_out) {
  if (!s) return VSO_E_INVALID_ARG;
  if (n_in) *n_in = (int)s->in_names.size();
  if (n_out) *n_out = (int)s->out_names.size();
  return VSO_OK;
}

static int copy_name(const std::vector<std::string>& v, int i, char* buf, int cap) {
  if (i < 0 || i >= (int)v.size() || !buf || cap < 1) return VSO_E_INVALID_ARG;
  std::snprintf(buf, (size_t)cap, "%s", v[i].c_str());
  return (int)v[i].size();
}

static int copy_shape(const std::vector<std::vector<int64_t>>& v, int i, int64_t* dims, int cap) {
  if (i < 0 || i >= (int)v.size() || !dims) return VSO_E_INVALID_ARG;
  const int n = (int)v[i].size();
  for (int k = 0; k < n && k < cap; ++k) dims[k] = v[i][k];
  return n;
}

int vso_input_name(const vso_session* s, int i, char* buf, int cap) { return s ? copy_name(s->in_names, i, buf, cap) : VSO_E_INVALID_ARG; }
int vso_output_name(const vso_session* s, int i, char* buf, int cap) { return s ? copy_name(s->out_names, i, buf, cap) : VSO_E_INVALID_ARG; }
int vso_input_shape(const vso_session* s, int i, int64_t* dims, int cap) { return s ? copy_shape(s->in_shapes, i, dims, cap) : VSO_E_INVALID_ARG; }
int vso_output_shape(const vso_session* s, int i, int64_t* dims, int cap) { return s ? copy_shape(s->out_shapes, i, dims, cap) : VSO_E_INVALID_ARG; }
int vso_output_type(const vso_session* s, int i) {
  return s && i >= 0 && i < (int)s->out_types.size() ? s->out_types[i] : VSO_E_INVALID_ARG;
}

// inputs -> the session's tensors, the launch list, the outputs back, all on
// `st`; host: the callers' pointers are host memory, and the call waits
static int run_on(vso_session* s, const float* const* inputs, float* const* outputs, hipStream_t st, bool host) {
  if (!s) return fail_s(nullptr, VSO_E_INVALID_ARG, "null session");
  if (!inputs || !outputs) return fail_s(s, VSO_E_INVALID_ARG, "null inputs/outputs");
  Busy b(s);
  if (!b.ok) return fail_s(s, VSO_E_INVALID_ARG, "a run is already in flight on this session");
  if (hipSetDevice(s->device) != hipSuccess) return fail_s(s, VSO_E_HIP, "hipSetDevice failed");
  if (!st) st = s->stream;
  for (size_t k = 0; k < s->in_bufs.size(); ++k) {
    if (host && !inputs[k]) return fail_s(s, VSO_E_INVALID_ARG, "null input " + std::to_string(k));
    if (hipMemcpyAsync(s->bufs[s->in_bufs[k]], inputs[k], numel(s->in_shapes[k]) * 4,
                       host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st) != hipSuccess)
      return fail_s(s, VSO_E_HIP, "input copy failed");
  }
  int rc = run_graph(s, st);
  if (rc) return rc;
  for (size_t k = 0; k < s->out_bufs.size(); ++k) {
    if (host && !outputs[k]) return fail_s(s, VSO_E_INVALID_ARG, "null output " + std::to_string(k));
    if (hipMemcpyAsync(outputs[k], s->bufs[s->out_bufs[k]], numel(s->out_shapes[k]) * 4,
                       host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st) != hipSuccess)
      return fail_s(s, VSO_E_HIP, "output copy failed");
  }
  if (host && hipStreamSynchronize(st) != hipSuccess) return fail_s(s, VSO_E_HIP, "run failed");
  return VSO_OK;
}

int vso_run(vso_session* s, const float* const* inputs, float* const* outputs) {
  return run_on(s, inputs, outputs, nullptr, true);
}

int vso_run_device(vso_session* s, const float* const* d_inputs, float* const* d_outputs, void* stream) {
  return run_on(s, d_inputs, d_outputs, static_cast<hipStream_t>(stream), false);
}

int vso_launch_count(const vso_session* s) { return s ? (int)s->launches.size() : VSO_E_INVALID_ARG; }

int vso_tile_conv_count(const vso_session* s) { return s ? s->tile_convs : VSO_E_INVALID_ARG; }
int vso_ir_block_count(const vso_session* s) { return s ? s->ir_blocks : VSO_E_INVALID_ARG; }
int vso_attn_count(const vso_session* s) { return s ? s->attn_nodes : VSO_E_INVALID_ARG; }
int vso_head_count(const vso_session* s) { return s ? s->head_nodes : VSO_E_INVALID_ARG; }
int vso_qconv_count(const vso_session* s) { return s ? s->qconv_nodes : VSO_E_INVALID_ARG; }
int vso_dynq_count(const vso_session* s) { return s ? s->dynq_nodes : VSO_E_INVALID_ARG; }
int vso_lane_count(const vso_session* s) { return s ? (s->graph ? s->lanes_used : 0) : VSO_E_INVALID_ARG; }

int vso_launch_name(const vso_session* s, int k, char* buf, int cap) {
  if (!s || k < 0 || k >= (int)s->launches.size() || !buf || cap < 1) return VSO_E_INVALID_ARG;
  std::snprintf(buf, (size_t)cap, "%s", s->launches[k].name.c_str());
  return (int)s->launches[k].name.size();
}

}  // extern "C"
