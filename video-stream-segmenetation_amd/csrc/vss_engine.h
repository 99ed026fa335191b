// vss_engine.h — what the C ABI's compile units share (internal, not installed).
//
// vss_capi.hip is the engine: planner, slots, graphs, forward, the queued host
// path.  The feature objects live in units of their own — vss_capi_post.hip
// (vss_post_state, compositing, vss_post_pool), vss_capi_background.hip
// (vss_background, matte, layers), vss_capi_video.hip (vss_video),
// vss_capi_streams.hip (the calls over many streams, which use all three) — and
// see the engine through this header.  Everything here is in vss_engine, a namespace of
// hidden visibility: none of it enters the library's export table.
// Slot and vss_handle change layout under -DVSS_TRACE, so the trace library
// compiles every unit that includes this header with it (Makefile: CAPI_UNITS).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/vss.h"
#include "vss_kernels.h"

namespace vss_engine __attribute__((visibility("hidden"))) {

using namespace vss;

struct Rec {
  uint32_t kind, cin, chid, cout, stride, flags, src, skip, off[8];
};

struct LayerPlan {
  Rec rec{};
  int C = 0, H = 0, W = 0;     // output shape
  int inH = 0, inW = 0;        // shape of rec.src's output (x)
  int mode = -1, stride = 1, chid = 0;
  int TH = 0, TW = 0, tiles_x = 0, tiles_y = 0;
  int flags = 0;
  int ks = 1, xp = 1, sp = 1;  // hidden split of this layer, parts of its x / skip (block_flags)
  size_t part_stride = 0;      // floats between the parts of an activation
  long wimg_stride = 0;        // floats between the slices' weight images
  size_t lds = 0;
  const BlockEntry* entry = nullptr;  // compiled shape (registry)
  const BlockEntry* small = nullptr;  // the autotuner's batch-1 pick, for forwards of <= small_tile_n frames
  bool fused = false;          // computed inside its only consumer's prologue (no launch of its own)
  int acc_off = -1;            // DEC: offset of its [kAccSlots][2][C] norm accumulator in a frame's row
  const float* wimg = nullptr;  // LDS weight image (block_lds regions w1..b2)
  const char* wfrag = nullptr;  // expand layers: the chunks' fragment records (expand_frag), slice after slice
  long wfrag_stride = 0;        // bytes between the slices' records
  const float *gamma = nullptr, *beta = nullptr;
  const float *stem_w = nullptr, *stem_b = nullptr, *head_w = nullptr;
  float head_b = 0.f;
};

// One kernel launch of the forward: function, grid, LDS and its parameter
// block (every kernel takes one parameter struct by value).
struct Launch {
  const void* fn = nullptr;
  dim3 grid;
  int threads = kThreads;
  size_t lds = 0;
  int layer = 0;
  union Prm {
    StemParams stem;
    BlockParams block;
    HeadParams head;
  } prm;
};

// A forward's executable graphs per (slot, shape): up to kExecPerShape
// executables, each bound to the caller buffers (frames, masks) it last ran
// with.  A call whose buffers match one replays it as is; otherwise a new
// executable is built while the set has room, and after that the least
// recently used one is patched (hipGraphExecKernelNodeSetParams on the kernel
// nodes whose parameters differ — the first layer reads the frames, the head
// writes the masks) once the slot's latest work is done: the slot's done event,
// which every call records after its launch anyway (release_slot), completes
// after every launch of every executable of the slot, so the executables keep
// no event of their own — one event record, one barrier packet, per call
// instead of two.  Callers rotating up to kExecPerShape buffer pairs through a
// slot never patch in steady state, so they never wait here (the
// round-3 single executable waited on every call of a caller rotating 3
// buffers over 4 slots, holding the handle's lock); a caller rotating more
// pairs than that patches on every call and waits for the slot's previous call.
using GraphKey = std::tuple<int, int, int, int, size_t, size_t>;  // n, fh, fw, fc, row / frame stride
constexpr int kExecPerShape = 4;
struct GraphEntry {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool launched = false;              // ever launched: the slot's done event then covers it
  unsigned long long tick = 0;        // LRU clock of its latest launch
  std::vector<hipGraphNode_t> nodes;  // one kernel node per launch, in order
  std::vector<Launch> launches;       // the parameters the executable graph holds now
};

// The rows of an fh-row frame that the tfjs-legacy resize to the model's rows
// reads (prep_tap's y0 / y1, the same float arithmetic), for the queued host
// path's row staging (vss_stage.hip).
struct RowPlan {
  std::vector<int> rows;                    // sorted, distinct
  std::vector<std::pair<int, int>> runs;    // [first, last + 1) runs of consecutive rows
  int* d_rows = nullptr;                    // device copy of rows
};

// One batch in flight on one GPU: everything a forward writes.
struct Slot {
  std::vector<float*> act;            // per layer: [ks][max_batch][H][W][C]
  unsigned long long* acc = nullptr;  // decoder instance-norm accumulators [max_batch][acc_stride]
  float* d_masks = nullptr;           // [max_batch][P]: host paths' masks (the all-gather's send buffer)
  float* d_gather = nullptr;          // RCCL handles: [nranks * max_batch][P]
  hipStream_t stream = nullptr;       // the slot's stream (queued host calls)
  hipEvent_t done = nullptr;          // recorded after the slot's latest work (host or device call)
  hipStream_t done_stream = nullptr;  // the stream `done` was last recorded on
  hipEvent_t host_done = nullptr;     // engine 0: recorded after the latest host batch's D2H
  bool used = false;
  // Host-side state of the slot's latest host batch (guarded by the handle's mu):
  bool leased = false;                // reserved by vss_staging_acquire for its holder's next call
  bool host_busy = false;             // a host batch whose completion (copy / callback /
                                      // synchronous wait) has not finished; the slot's pinned
                                      // buffers belong to it until then
  int status = VSS_OK;                // of the latest host batch
  vss_ticket ticket = ~0ull;          // latest host ticket that ran in this slot (device calls
                                      // take no ticket and leave it alone)
  bool stem_stored = false;           // the latest forward stored the fused stem (VSS_OPT_KEEP_STEM)
  std::map<GraphKey, std::vector<GraphEntry>> graphs;
  std::map<GraphKey, unsigned long long> shape_tick;  // per shape: graph_tick of its latest use
  unsigned long long graph_tick = 0;
#ifdef VSS_TRACE
  std::vector<unsigned long long*> trace;  // per layer, [workgroups][16] stamps of this slot's latest forward
#endif
  ncclComm_t comm = nullptr;          // this GPU's communicator of the slot (RCCL handles)
  // host-path staging, allocated on the slot's first host call
  uint8_t* d_frames = nullptr;
  uint8_t* h_frames = nullptr;        // pinned
  float* h_masks = nullptr;           // pinned [max_batch][P] (engine 0: the whole batch)
  float* d_fmasks = nullptr;          // VSS_OUT_FRAME: [max_batch][frame] masks
  float* h_fmasks = nullptr;
};

class CopyPool;  // host threads for the pinned staging copies (vss_capi.hip)
constexpr long kDefaultKsplitPixels = 256;

}  // namespace vss_engine

struct vss_handle {
  using Rec = vss_engine::Rec;
  using LayerPlan = vss_engine::LayerPlan;
  using RowPlan = vss_engine::RowPlan;
  using Slot = vss_engine::Slot;
  vss_config cfg{};            // this engine's config (max_batch = its share of the handle's)
  std::string weights_path;
  // the last error: written by any thread that fails a call (several may
  // submit at once) and by the completion thread; read by vss_last_error,
  // which copies it under err_mu into the caller's thread-local buffer
  std::string err;
  mutable std::mutex err_mu;
  int device = 0;
  hipStream_t stream = nullptr;          // NULL-stream device calls, post / composite, autotune
  std::vector<Rec> recs;
  std::vector<float> hdata;
  float eps = 1e-5f;
  std::vector<LayerPlan> L;
  int acc_stride = 0;
  std::vector<void*> dev_allocs;
  std::vector<void*> host_allocs;
  size_t dev_bytes = 0;
  size_t frame_cap = 0;        // staging bytes per slot
  std::vector<Slot> slots;
  int last_slot = -1;          // slot of the latest forward (vss_read_layer)
  std::map<int, RowPlan> row_plans;  // by frame height
  int row_fetch = 1;           // VSS_OPT_ROW_FETCH
#ifdef VSS_TRACE
  std::vector<int> trace_wgs;              // workgroups of the layer's last launch
#endif
  uint8_t* d_comp = nullptr;      // vss_segment_composite / _background output, allocated on first use
  std::atomic<size_t> bg_bytes{0};  // device buffers of the handle's vss_background and vss_video objects
  float* d_post_alpha = nullptr;  // vss_segment_post outputs [max_batch][P]
  uint8_t* d_post_u8 = nullptr;
  int use_graph = 1;
  int profile = 0;
  int fuse_stem = 1;              // env VSS_FUSE_STEM=0: launch the stem on its own
  int keep_stem = 0;              // VSS_OPT_KEEP_STEM: the fused stem also stores its activation
  // expand layers with at most this many output pixels per frame split their
  // hidden channels over ks_max() workgroups (env VSS_KSPLIT_PIXELS overrides)
  long ksplit_pixels = vss_engine::kDefaultKsplitPixels;
  // The hidden-channel split (KS workgroups per tile of a deep low-res expand
  // layer, consumers summing the parts) buys latency with one batch in flight
  // and costs throughput with four: measured round 4 (profiles/r04a/session.txt,
  // two interleaved pairs): headline 206.9 / 206.1k without against 194.7 /
  // 203.7k with, batch sweep at 4 in flight +4 % (b8), +7.5 % (b32), +6 % (b64),
  // at 1 in flight -3 % (b8).  Off by default; env VSS_KSPLIT=1 turns it on.
  bool ksplit_on = false;
  // profiling: ring of event pairs per layer
  static constexpr int kProfRing = 32;
  std::vector<hipEvent_t> ev;  // [ring][layer][2]
  std::vector<int> ring_pending;
  int prof_next = 0;
  std::vector<double> prof_sum;
  int prof_count = 0;
  int last_n = 0;
  // ---- the handle (engine 0 only) ----
  std::vector<vss_handle*> peers;  // engines 1..R-1 (device_ids[1..])
  int user_max_batch = 0;          // the handle's max_batch (all GPUs)
  bool rccl = false;               // host calls all-gather over RCCL (device_ids given)
  int nranks = 1, rank = 0;        // vss_comm_init_rank clique (one GPU per process)
  // set (release) once every communicator of the clique exists: the lock-free
  // vss_comm_status reads the communicators only after seeing it (acquire)
  std::atomic<bool> clique{false};
  // VSS_OPT_GATHER_FORM, fixed at vss_comm_init_rank.  VSS_GATHER_ORDERED (the
  // default): the clique's all-gathers on one communicator (slot 0's, the only
  // one created) and one stream, events ordering each gather after its forward
  // and the caller's stream after the gather — one total order of collectives
  // per rank.  VSS_GATHER_CONCURRENT: each slot's own communicator on the
  // slot's stream (vss_segment_gather_device)
  int gather_form = VSS_GATHER_ORDERED;
  std::vector<hipEvent_t> gather_ev;  // the ordered form's gather-done events, a ring of 2 x depth (call % size)
  // Submissions (slot choice, staging, enqueue) are serialised by mu; no
  // thread holds it while it waits for the GPU (waiters drop it first).
  std::mutex mu;
  std::condition_variable slot_cv;   // a slot's host_busy went false
  std::mutex post_mu;              // the synchronous post / composite calls share scratch
  vss_ticket next_ticket = 0;      // host batches (vss_submit*, vss_segment*)
  unsigned long long device_calls = 0;  // vss_segment_device: slot = count % depth
  int small_tile_n = 0;            // forwards of at most this many frames use LayerPlan::small
  std::atomic<unsigned long long> gather_calls{0};  // vss_segment_gather_device: slot = count % depth
                                                   // (atomic: vss_comm_status reads it lock-free)
  long graph_builds = 0, graph_patches = 0;  // VSS_OPT_GRAPH_BUILDS / _PATCHES
  vss_engine::CopyPool* pool = nullptr;
  // The completion thread (started on the first host batch that needs one):
  // waits for the queued host batches in ticket order, copies their masks
  // from the slot's pinned buffer into the caller's memory, fires callbacks.
  struct Completion {
    vss_ticket ticket;
    int slot;
    float* out;          // null: the D2H already went to the caller's pinned block
    const float* src;
    size_t bytes;
    vss_callback cb;
    void* user;
  };
  std::thread done_thread;
  std::mutex done_mu;
  std::condition_variable done_cv;
  std::deque<Completion> done_q;
  bool done_stop = false;
};

#define HIP_TRY(h, expr)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((h), e_ == hipErrorOutOfMemory ? VSS_E_OOM : VSS_E_HIP,                \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                     \
  } while (0)

namespace vss_engine __attribute__((visibility("hidden"))) {

// ---- the engine (vss_capi.hip) ----
extern thread_local std::string g_tls_error;  // the last error of calls without a handle
void set_err(vss_handle* h, const std::string& msg);
int fail(vss_handle* h, int code, const std::string& msg);
int check_frames(vss_handle* h, int n, int fh, int fw, int fc, size_t rs, size_t fs, int max_n);
int seam_on_stream(vss_handle* h, std::unique_lock<std::mutex>& lk, const uint8_t* frames, int n, int fh, int fw,
                   int fc, size_t rs, int* slot);
int finish_seam(vss_handle* h, std::unique_lock<std::mutex>& lk, int k, int rc);
int segment_device_on(vss_handle* h, int* slot, const uint8_t* d_frames, int n, int height, int width, int channels,
                      size_t row_stride, size_t frame_stride, float* d_masks, void* stream)
    __attribute__((always_inline));

template <class T>
int dalloc(vss_handle* h, T** p, size_t bytes) {
  void* q = nullptr;
  bytes = std::max<size_t>(bytes, 16);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(h, VSS_E_OOM, "hipMalloc(" + std::to_string(bytes) + ") failed");
  h->dev_allocs.push_back(q);
  h->dev_bytes += bytes;
  *p = static_cast<T*>(q);
  return VSS_OK;
}

// ---- what the units say once ----
// the most frames a device call takes: the handle's max_batch over all GPUs
inline int max_frames(const vss_handle* h) { return std::max(h->cfg.max_batch, h->user_max_batch); }
// a call's stream argument: null means the handle's stream
inline hipStream_t stream_or(const vss_handle* h, void* stream) {
  return stream ? static_cast<hipStream_t>(stream) : h->stream;
}
// after the launches of `what`: the launch error, if any
inline int launched(vss_handle* h, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, VSS_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return VSS_OK;
}

// an RGBA batch's geometry; strict: the frame stride is a multiple of 4 as well
inline bool rgba_geometry_ok(const uint8_t* p, size_t rs, size_t fs, int fh, int fw, bool strict) {
  return rs >= (size_t)fw * 4 && rs % 4 == 0 && fs >= rs * (size_t)fh && (!strict || fs % 4 == 0) &&
         !(reinterpret_cast<uintptr_t>(p) & 3);
}

// (re)allocate one device buffer of a background, video or pool object to
// `bytes` (0: free it); these buffers count into vss_info.device_bytes
template <class T>
int counted_alloc(vss_handle* h, T** p, size_t* have, size_t bytes) {
  if (*p) {
    (void)hipFree(*p);
    h->bg_bytes -= *have;
    *p = nullptr;
    *have = 0;
  }
  if (!bytes) return VSS_OK;
  void* q = nullptr;
  if (hipMalloc(&q, bytes) != hipSuccess) return fail(h, VSS_E_OOM, "hipMalloc(" + std::to_string(bytes) + ") failed");
  *p = static_cast<T*>(q);
  *have = bytes;
  h->bg_bytes += bytes;
  return VSS_OK;
}

// The "latest call" fence of an object whose calls share device scratch
// (vss_background, vss_video, vss_post_pool; the object's mu held): an event
// recorded after the object's latest call.  A call on another stream waits for
// it on the device; the host waits for it (quiesce) before a buffer the call
// may use is freed, reallocated or rewritten.
//
// A call over several objects (include/vss_streams.h) records ONE event, its
// first object's, and the others follow it: an event record costs the device
// about 4.8 us, eight of them more than the composite itself.
// So the event sits in a box that outlives its object while another follows it.
// Following stays correct when the box is recorded again: its owner records
// only on a stream that waited for its own latest call, so every later record
// of a box completes after all the earlier ones.
struct Fence {
  struct Box {
    hipEvent_t event = nullptr;
    ~Box() {
      if (event) (void)hipEventDestroy(event);
    }
  };
  std::shared_ptr<Box> own;     // the event this object records
  std::shared_ptr<Box> latest;  // the event that covers this object's latest call: own, or the one it follows
  hipStream_t last_stream = nullptr;
  bool used = false;
  hipError_t create() {
    latest = own = std::make_shared<Box>();
    return hipEventCreateWithFlags(&own->event, hipEventDisableTiming);
  }
  void destroy() {
    latest.reset();
    own.reset();
  }
  int wait_on(vss_handle* h, hipStream_t s) const {
    if (used && last_stream != s) HIP_TRY(h, hipStreamWaitEvent(s, latest->event, 0));
    return VSS_OK;
  }
  int record(vss_handle* h, hipStream_t s) {
    HIP_TRY(h, hipEventRecord(own->event, s));
    latest = own;
    last_stream = s;
    used = true;
    return VSS_OK;
  }
  // this object's latest call is the one `leader` has just recorded
  void follow(const Fence& leader) {
    latest = leader.latest;
    last_stream = leader.last_stream;
    used = true;
  }
  int quiesce(vss_handle* h) const {
    HIP_TRY(h, hipSetDevice(h->device));
    if (used) HIP_TRY(h, hipEventSynchronize(latest->event));
    return VSS_OK;
  }
};

// Bilateral weights as the reference computes them (Math.exp of the same
// double quotients); built on the host so they are the exact doubles the
// oracle's libm produces.  Shared by vss_post_state and vss_post_pool.
constexpr int kRangeTab = 3 * 255 * 255 + 1;
struct PostTables {
  double* rtab = nullptr;   // device: exp(-r / (2 sigma_r^2)), r in [0, 3*255^2]; its owner allocates and frees it
  double sw[3] = {0, 0, 0};
  double tab_sigma = -1.0;  // the sigma_range rtab holds
  bool update(const vss_post_config& c);  // sw, and rtab when sigma_range changed; false: the upload failed
};

}  // namespace vss_engine

// ---- the feature objects more than one unit sees ----
struct vss_post_state {
  vss_handle* h = nullptr;
  vss_post_config cfg{};
  float* state = nullptr;   // [P] prevAlpha
  int* valid = nullptr;     // device flag: 0 before the stream's first frame
  float* ema = nullptr;     // [max_batch][P]
  float* state2 = nullptr;  // [P] the other prevAlpha buffer (the stabilised EMA reads one, writes the other)
  vss::FaceFrame* d_faces = nullptr;       // [max_batch] face inputs set by vss_post_set_faces
  const vss::FaceFrame* faces = nullptr;   // the next call's face inputs (d_faces or a caller's device array)
  int faces_n = 0;                         // ... for this many frames (0: none)
  vss_engine::PostTables tab;
};

struct vss_background {
  vss_handle* h = nullptr;
  std::mutex mu;                 // setters and composites of one object are serialised
  int mode = VSS_BG_COLOR;
  uint32_t color = 32u | (32u << 8) | (32u << 16);  // u2FrameProc.ts:89
  uint8_t* d_src = nullptr;      // IMAGE: the user's image [sh][sw][sc], tight rows
  int sh = 0, sw = 0, sc = 0;
  size_t src_bytes = 0;
  uint8_t* d_img = nullptr;      // IMAGE: d_src scaled to img_fh x img_fw (0: not built)
  int img_fh = 0, img_fw = 0;
  size_t img_bytes = 0;
  uint32_t* d_hblur = nullptr;   // BLUR: the horizontal pass's output, grown on demand
  size_t hblur_bytes = 0;
  int radius = 0;
  uint16_t w[vss::kBlurMaxRadius + 1] = {};  // taps 0 (centre) .. radius
  uint16_t* d_taps = nullptr;    // w on the device, for the calls over many streams (vss_background_set_blur)
  size_t taps_bytes = 0;
  int refine_radius = 0;         // the edge-aware matte: 0 = off
  double refine_eps = 0.0;
  uint8_t* d_matte = nullptr;    // its planes for n frames: (abar, bbar), (a_q, b_q), L; grown on demand
  size_t matte_bytes = 0;
  // branding layers (include/vss_layers.h)
  struct Layer {
    vss_layer l;                 // pixels = null: the sprite lives in d_sprites
    size_t sprite_off;           // IMAGE: byte offset of its premultiplied copy
  };
  std::vector<Layer> layers;
  int canvas_w = 1920, canvas_h = 1080;  // customization.ts:37
  int level = 2;                 // 'medium', customization.ts:28
  uint8_t* d_sprites = nullptr;  // every IMAGE layer's sprite, premultiplied RGBA, tight rows
  size_t sprites_bytes = 0;
  uint32_t* d_plate = nullptr;   // the overlay O at plate_fh x plate_fw (0: not built), rows of layer_pitch dwords
  int plate_fh = 0, plate_fw = 0;
  size_t plate_bytes = 0;
  uint8_t* d_shadow = nullptr;   // the shadows' two u8 planes, [2][fh][layer_pitch]
  size_t shadow_bytes = 0;
  int img_mode = -1;             // what d_img holds: the mode it was built for,
  bool img_layered = false;      // whether O is baked into it,
  uint32_t img_color = 0;        // and (COLOR) from which colour
  bool img_for_image = false;    // d_img has served image mode (else it exists for a colour under layers only)
  vss_engine::Fence fence;       // recorded after every composite
};

// the post chain over many streams (vss_post.hip k_post_pool; include/vss_pool.h)
struct vss_post_pool {
  vss_handle* h = nullptr;
  std::mutex mu;                  // calls, resets and setters of one pool are serialised
  vss_post_config cfg{};
  int capacity = 0;
  float* planes = nullptr;        // [capacity][2][P] prevAlpha, double-buffered per stream
  size_t planes_bytes = 0;
  vss_engine::PostTables tab;     // one range table for every stream
  size_t rtab_bytes = 0;
  std::vector<uint8_t> seen;      // per stream: it has seen a frame (prevAlpha exists)
  std::vector<uint8_t> cur;       // per stream: the plane that holds its prevAlpha
  std::vector<uint64_t> stamp;    // per stream: the last call that named it (duplicate ids)
  uint64_t calls = 0;
  vss_engine::Fence fence;        // recorded after every call
};

// NV12 video I/O (vss_video.hip; include/vss_video.h)
struct vss_video {
  vss_handle* h = nullptr;
  std::mutex mu;                 // setters and calls of one object are serialised
  int std_ = VSS_CSC_BT709_LIMITED;
  uint8_t* d_buf = nullptr;      // RGBA in | RGBA out (px_cap pixels each) | masks f32 | alpha u8 (max_batch frames)
  size_t buf_bytes = 0, px_cap = 0;
  uint8_t* d_nv = nullptr;       // the host call's device planes: Y in | UV in | Y out | UV out
  size_t nv_bytes = 0;
  int slot = -1;                 // the handle slot whose executable graph is bound to d_buf (taken by the first call)
  vss_engine::Fence fence;       // recorded after every call
};

namespace vss_engine __attribute__((visibility("hidden"))) {

// ---- vss_capi_post.hip ----
// p->mu held.  What a pooled call may be refused for, before anything is enqueued.
int pool_check(vss_post_pool* p, const int* ids, int n, const uint8_t* d_frames, int fh, int fw, int fc, size_t rs,
               size_t fs, int max_n);
// p->mu held; arguments checked.  ceil(n / kPoolFrames) launches and the ordering event.
int pool_enqueue(vss_post_pool* p, const int* ids, int n, const uint8_t* d_frames, int fh, int fw, int fc, size_t rs,
                 size_t fs, const float* d_masks, const vss::FaceFrame* d_faces, float* d_alpha, uint8_t* d_u8,
                 hipStream_t s);
// the post chain for n frames on s (the state's stream order is the caller's)
int post_enqueue(vss_post_state* st, const uint8_t* d_frames, int n, int fh, int fw, int fc, size_t rs, size_t fs,
                 const float* d_masks, float* d_alpha, uint8_t* d_u8, hipStream_t s);
// frames fh x fw x fc and an alpha plane H x W onto an output of row / frame strides ors / ofs
void composite_params(CompositeParams* c, const uint8_t* d_frames, int fh, int fw, int fc, size_t rs, size_t fs,
                      const uint8_t* d_alpha, int H, int W, uint8_t* d_out, size_t ors, size_t ofs);
// The RGBA host calls' tail (h->post_mu and h->mu held).  comp_reserve, before
// the seam: h->d_comp exists and holds `bytes`.  comp_to_host, after an enqueue
// of status rc: the D2H of `bytes` on the handle's stream; returns the status.
int comp_reserve(vss_handle* h, size_t bytes);
int comp_to_host(vss_handle* h, int rc, uint8_t* out_rgba, size_t bytes);

// ---- vss_capi_background.hip ----
// bg->mu held: the composite over the background for n frames on s
int bg_enqueue(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int fh, int fw, int fc, size_t rs,
               size_t fs, const uint8_t* d_alpha, uint8_t* d_out, size_t ors, size_t ofs, hipStream_t s);

// One frame per stream, frame t over bgs[t] (include/vss_streams.h).  The
// distinct objects of a call, locked in address order: two calls that name the
// same objects in different orders cannot deadlock.  bgs: n non-null pointers.
struct BgStreamsLock {
  std::vector<vss_background*> objs;  // distinct, ascending
  BgStreamsLock(vss_background* const* bgs, int n) : objs(bgs, bgs + n) {
    std::sort(objs.begin(), objs.end(), std::less<vss_background*>());
    objs.erase(std::unique(objs.begin(), objs.end()), objs.end());
    for (vss_background* b : objs) b->mu.lock();
  }
  ~BgStreamsLock() {
    for (auto it = objs.rbegin(); it != objs.rend(); ++it) (*it)->mu.unlock();
  }
  BgStreamsLock(const BgStreamsLock&) = delete;
  BgStreamsLock& operator=(const BgStreamsLock&) = delete;
};
// no lock needed: bgs and its n entries are non-null objects of h
int bg_streams_args(vss_handle* h, vss_background* const* bgs, int n);
// the objects' mutexes held: what their settings refuse for frames fh x fw, before anything is enqueued
int bg_streams_check(vss_handle* h, vss_background* const* bgs, int n, int fh, int fw);
// the objects' mutexes held (lk), bg_streams_check passed: the composites on s, and each object's fence
int bg_streams_enqueue(vss_handle* h, const BgStreamsLock& lk, vss_background* const* bgs, int n,
                       const uint8_t* d_frames, int fh, int fw, int fc, size_t rs, size_t fs, const uint8_t* d_alpha,
                       uint8_t* d_out, size_t ors, size_t ofs, hipStream_t s);

// ---- vss_capi_video.hip ----
// one NV12 batch's geometry; `what` names the planes in the message
int check_nv12(vss_handle* h, const char* what, const uint8_t* y, size_t yp, size_t yfs, const uint8_t* uv, size_t up,
               size_t ufs, int n, int fh, int fw, int max_n);
vss::Nv12Params nv12_params(int std, const uint8_t* y, size_t yp, size_t yfs, const uint8_t* uv, size_t up, size_t ufs,
                            const uint8_t* rgba, size_t rs, size_t fs, int fh, int fw);
// v->mu held: v's scratch holds n frames fh x fw (it is regrown once v's latest call has ended)
int video_reserve(vss_video* v, int n, int fh, int fw);

}  // namespace vss_engine
