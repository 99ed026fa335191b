// vss_capi_post.hip — the C ABI of the post-processing chain (vss_post.hip):
// vss_post_state, compositing (k_composite) and vss_post_pool
// (include/vss_pool.h), over the engine in vss_capi.hip (vss_engine.h).
#include <cmath>

#include "vss_engine.h"

using namespace vss;
using namespace vss_engine;

bool PostTables::update(const vss_post_config& c) {
  const double ts2 = 2.0 * c.sigma_spatial * c.sigma_spatial, tr2 = 2.0 * c.sigma_range * c.sigma_range;
  for (int k = 0; k < 3; ++k) sw[k] = std::exp(-(double)k / ts2);
  if (tab_sigma != c.sigma_range) {
    std::vector<double> t(kRangeTab);
    for (int r = 0; r < kRangeTab; ++r) t[r] = std::exp(-(double)r / tr2);
    if (hipMemcpy(rtab, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return false;
    tab_sigma = c.sigma_range;
  }
  return true;
}

namespace {

int post_tables(vss_post_state* st) {
  if (!st->tab.update(st->cfg)) return fail(st->h, VSS_E_HIP, "post: table upload failed");
  return VSS_OK;
}

// the filter's parameters that do not depend on where the EMA comes from
void post_filter_params(PostFilterParams* pf, const vss_handle* h, const vss_post_config& c, const PostTables& tab,
                        int fh, int fw, int fc, size_t rs, size_t fs) {
  const int H = h->cfg.model_h, W = h->cfg.model_w;
  pf->row_stride = (long)rs;
  pf->frame_stride = (long)fs;
  pf->fh = fh; pf->fw = fw; pf->fc = fc;
  pf->ry = (float)((double)fh / (double)H);
  pf->rx = (float)((double)fw / (double)W);
  pf->H = H; pf->W = W;
  pf->rtab = tab.rtab;
  for (int k = 0; k < 3; ++k) pf->sw[k] = tab.sw[k];
  pf->lo = c.noise_cutoff;
  pf->hi = c.high_threshold;
  pf->denom = std::max(1e-6, c.high_threshold - c.noise_cutoff);
  pf->gamma = c.gamma;
  pf->use_bilateral = c.use_bilateral;
}

// The synchronous alpha calls' tail (h->post_mu and h->mu held).  Their device
// outputs are the handle's d_post_alpha / d_post_u8, each only where the caller
// asked for that plane (alpha_planes); alpha_to_host, after an enqueue of status
// rc, copies n frames of those to the host on the handle's stream and returns
// the status.
struct AlphaPlanes {
  float* f32;
  uint8_t* u8;
};
AlphaPlanes alpha_planes(const vss_handle* h, const float* out, const uint8_t* out_u8) {
  return {out ? h->d_post_alpha : nullptr, out_u8 ? h->d_post_u8 : nullptr};
}
int alpha_to_host(vss_handle* h, int rc, int n, float* out, uint8_t* out_u8) {
  if (rc) return rc;
  const size_t P = (size_t)h->cfg.model_h * h->cfg.model_w;
  const AlphaPlanes d = alpha_planes(h, out, out_u8);
  hipError_t e = hipSuccess;
  if (out) e = hipMemcpyAsync(out, d.f32, (size_t)n * P * 4, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && out_u8) e = hipMemcpyAsync(out_u8, d.u8, (size_t)n * P, hipMemcpyDeviceToHost, h->stream);
  if (e != hipSuccess) return fail(h, VSS_E_HIP, std::string("D2H: ") + hipGetErrorString(e));
  return VSS_OK;
}

}  // namespace

int vss_engine::post_enqueue(vss_post_state* st, const uint8_t* d_frames, int n, int fh, int fw, int fc, size_t rs,
                             size_t fs, const float* d_masks, float* d_alpha, uint8_t* d_u8, hipStream_t s) {
  vss_handle* h = st->h;
  const int H = h->cfg.model_h, W = h->cfg.model_w;
  const FaceFrame* faces = nullptr;
  if (st->faces_n) {
    if (st->faces_n != n)
      return fail(h, VSS_E_INVALID_ARG, "vss_post_set_faces was given " + std::to_string(st->faces_n) +
                                            " frames, this call has " + std::to_string(n));
    faces = st->faces;
    st->faces_n = 0;  // consumed
    st->faces = nullptr;
  }
  if (faces) {
    // the stabilised EMA, one frame at a time (the warp reads prevAlpha at other pixels)
    for (int t = 0; t < n; ++t) {
      PostFaceEmaParams pe{};
      pe.mask = d_masks + (long)t * H * W;
      pe.prev = st->state;
      pe.next = st->state2;
      pe.ema = st->ema + (long)t * H * W;
      pe.valid = st->valid;
      pe.first = t == 0;
      pe.face = faces + t;
      pe.H = H;
      pe.W = W;
      pe.a = st->cfg.ema;
      launch_post_face_ema(pe, s);
      std::swap(st->state, st->state2);
    }
  } else {
    PostEmaParams pe{};
    pe.masks = d_masks;
    pe.ema = st->ema;
    pe.state = st->state;
    pe.valid = st->valid;
    pe.n = n;
    pe.P = (long)H * W;
    pe.a = st->cfg.ema;
    launch_post_ema(pe, s);
  }
  HIP_TRY(h, hipMemsetAsync(st->valid, 1, sizeof(int), s));  // the stream has seen its first frame
  PostFilterParams pf{};
  pf.faces = faces;
  pf.ema = st->ema;
  pf.frames = d_frames;
  post_filter_params(&pf, h, st->cfg, st->tab, fh, fw, fc, rs, fs);
  pf.alpha = d_alpha;
  pf.alpha_u8 = d_u8;
  launch_post_filter(pf, n, s);
  return launched(h, "post");
}

extern "C" {

void vss_post_config_default(vss_post_config* c) {
  if (!c) return;
  c->ema = 0.55;
  c->noise_cutoff = 0.06;
  c->high_threshold = 0.95;
  c->gamma = 0.4;
  c->sigma_spatial = 1.0;
  c->sigma_range = 12.0;
  c->use_bilateral = 1;
}

int vss_post_create(vss_handle* h, const vss_post_config* cfg, vss_post_state** out) {
  if (!h || !out) return fail(h, VSS_E_INVALID_ARG, "null handle/out");
  *out = nullptr;
  if (h->cfg.model_h < 3 || h->cfg.model_w < 3) return fail(h, VSS_E_UNSUPPORTED, "mask too small for post");
  vss_post_state* st = new vss_post_state();
  st->h = h;
  if (cfg) st->cfg = *cfg;
  else vss_post_config_default(&st->cfg);
  const size_t P = (size_t)h->cfg.model_h * h->cfg.model_w;
  const size_t nb = (size_t)max_frames(h);
  auto bail = [&](int rc) {
    vss_post_destroy(st);
    return rc;
  };
  HIP_TRY(h, hipSetDevice(h->device));
  if (hipMalloc(&st->state, P * 4) != hipSuccess || hipMalloc(&st->valid, 16) != hipSuccess ||
      hipMalloc(&st->ema, P * 4 * nb) != hipSuccess || hipMalloc(&st->state2, P * 4) != hipSuccess ||
      hipMalloc(&st->d_faces, sizeof(FaceFrame) * nb) != hipSuccess ||
      hipMalloc(&st->tab.rtab, (size_t)kRangeTab * 8) != hipSuccess)
    return bail(fail(h, VSS_E_OOM, "post: hipMalloc failed"));
  if (hipMemset(st->valid, 0, 16) != hipSuccess || hipMemset(st->state, 0, P * 4) != hipSuccess)
    return bail(fail(h, VSS_E_HIP, "post: hipMemset failed"));
  int rc = post_tables(st);
  if (rc) return bail(rc);
  *out = st;
  return VSS_OK;
}

void vss_post_destroy(vss_post_state* st) {
  if (!st) return;
  if (st->h) {
    (void)hipSetDevice(st->h->device);
    (void)hipDeviceSynchronize();
  }
  if (st->state) (void)hipFree(st->state);
  if (st->valid) (void)hipFree(st->valid);
  if (st->ema) (void)hipFree(st->ema);
  if (st->state2) (void)hipFree(st->state2);
  if (st->d_faces) (void)hipFree(st->d_faces);
  if (st->tab.rtab) (void)hipFree(st->tab.rtab);
  delete st;
}

int vss_post_reset(vss_post_state* st) {
  if (!st) return VSS_E_INVALID_ARG;
  HIP_TRY(st->h, hipSetDevice(st->h->device));
  HIP_TRY(st->h, hipDeviceSynchronize());
  HIP_TRY(st->h, hipMemset(st->valid, 0, sizeof(int)));
  st->faces_n = 0;
  st->faces = nullptr;
  return VSS_OK;
}

static_assert(sizeof(FaceFrame) == sizeof(vss_face_frame), "FaceFrame mirrors vss_face_frame");

int vss_post_set_faces(vss_post_state* st, const vss_face_frame* faces, int n) {
  if (!st) return VSS_E_INVALID_ARG;
  if (!faces || n < 1 || n > max_frames(st->h)) return fail(st->h, VSS_E_INVALID_ARG, "faces: 1..max_batch frames");
  HIP_TRY(st->h, hipSetDevice(st->h->device));
  HIP_TRY(st->h, hipMemcpyAsync(st->d_faces, faces, sizeof(FaceFrame) * n, hipMemcpyHostToDevice, st->h->stream));
  HIP_TRY(st->h, hipStreamSynchronize(st->h->stream));  // consumers may run on any stream
  st->faces = st->d_faces;
  st->faces_n = n;
  return VSS_OK;
}

int vss_post_set_faces_device(vss_post_state* st, const vss_face_frame* d_faces, int n) {
  if (!st) return VSS_E_INVALID_ARG;
  if (!d_faces || n < 1 || n > max_frames(st->h))
    return fail(st->h, VSS_E_INVALID_ARG, "faces: a device array of 1..max_batch frames");
  st->faces = reinterpret_cast<const FaceFrame*>(d_faces);
  st->faces_n = n;
  return VSS_OK;
}

int vss_post_set_config(vss_post_state* st, const vss_post_config* cfg) {
  if (!st || !cfg) return VSS_E_INVALID_ARG;
  if (cfg->sigma_spatial <= 0 || cfg->sigma_range <= 0) return fail(st->h, VSS_E_INVALID_ARG, "sigmas must be > 0");
  HIP_TRY(st->h, hipSetDevice(st->h->device));
  HIP_TRY(st->h, hipDeviceSynchronize());
  st->cfg = *cfg;
  return post_tables(st);
}

int vss_postprocess_device(vss_post_state* st, const uint8_t* d_frames, int n, int height, int width, int channels,
                           size_t row_stride, size_t frame_stride, const float* d_masks, float* d_alpha,
                           uint8_t* d_alpha_u8, void* stream) {
  if (!st) return fail(nullptr, VSS_E_INVALID_ARG, "null post state");
  vss_handle* h = st->h;
  if (!d_masks || (!d_frames && st->cfg.use_bilateral)) return fail(h, VSS_E_INVALID_ARG, "null device pointer");
  int rc = check_frames(h, n, height, width, channels, row_stride, frame_stride, max_frames(h));
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  return post_enqueue(st, d_frames, n, height, width, channels, row_stride, frame_stride, d_masks, d_alpha,
                      d_alpha_u8, stream_or(h, stream));
}

int vss_segment_post(vss_handle* h, vss_post_state* st, const uint8_t* frames, int n, int height, int width,
                     int channels, size_t row_stride, float* alpha_out, uint8_t* alpha_u8_out) {
  if (!h || !st || st->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / post state mismatch");
  if (!alpha_out && !alpha_u8_out) return fail(h, VSS_E_INVALID_ARG, "no output requested");
  std::lock_guard<std::mutex> pl(h->post_mu);
  std::unique_lock<std::mutex> lk(h->mu);
  int k = 0;
  int rc = seam_on_stream(h, lk, frames, n, height, width, channels, row_stride, &k);
  if (rc) return rc;
  const Slot& s = h->slots[k];
  const AlphaPlanes d = alpha_planes(h, alpha_out, alpha_u8_out);
  rc = post_enqueue(st, s.d_frames, n, height, width, channels, row_stride, row_stride * (size_t)height, s.d_masks,
                    d.f32, d.u8, h->stream);
  return finish_seam(h, lk, k, alpha_to_host(h, rc, n, alpha_out, alpha_u8_out));
}

}  // extern "C"

// ---- compositing (vss_post.hip k_composite) ---------------------------------
void vss_engine::composite_params(CompositeParams* c, const uint8_t* d_frames, int fh, int fw, int fc, size_t rs,
                                  size_t fs, const uint8_t* d_alpha, int H, int W, uint8_t* d_out, size_t ors,
                                  size_t ofs) {
  c->frames = d_frames;
  c->row_stride = (long)rs;
  c->frame_stride = (long)fs;
  c->fh = fh; c->fw = fw; c->fc = fc;
  c->alpha = d_alpha;
  c->H = H; c->W = W;
  c->sy = (float)c->H / (float)fh;
  c->sx = (float)c->W / (float)fw;
  c->out = d_out;
  c->out_row_stride = (long)ors;
  c->out_frame_stride = (long)ofs;
}

int vss_engine::comp_reserve(vss_handle* h, size_t bytes) {
  const size_t cap = (size_t)h->cfg.max_batch * h->cfg.max_frame_h * h->cfg.max_frame_w * 4;
  if (!h->d_comp) {
    int rc = dalloc(h, &h->d_comp, cap);
    if (rc) return rc;
  }
  if (bytes > cap)
    return fail(h, VSS_E_INVALID_ARG, "RGBA output exceeds the handle's capacity (max_batch, max_frame_h/w)");
  return VSS_OK;
}

int vss_engine::comp_to_host(vss_handle* h, int rc, uint8_t* out_rgba, size_t bytes) {
  if (rc) return rc;
  const hipError_t e = hipMemcpyAsync(out_rgba, h->d_comp, bytes, hipMemcpyDeviceToHost, h->stream);
  if (e != hipSuccess) return fail(h, VSS_E_HIP, std::string("D2H: ") + hipGetErrorString(e));
  return VSS_OK;
}

namespace {

int composite_enqueue(vss_handle* h, const uint8_t* d_frames, int n, int fh, int fw, int fc, size_t rs, size_t fs,
                      const uint8_t* d_alpha, uint8_t* d_out, size_t ors, size_t ofs, hipStream_t s) {
  CompositeParams p{};
  composite_params(&p, d_frames, fh, fw, fc, rs, fs, d_alpha, h->cfg.model_h, h->cfg.model_w, d_out, ors, ofs);
  launch_composite(p, n, s);
  return launched(h, "composite");
}

}  // namespace

extern "C" {

int vss_composite_device(vss_handle* h, const uint8_t* d_frames, int n, int height, int width, int channels,
                         size_t row_stride, size_t frame_stride, const uint8_t* d_alpha_u8, uint8_t* d_out_rgba,
                         size_t out_row_stride, size_t out_frame_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  if (!d_frames || !d_alpha_u8 || !d_out_rgba) return fail(h, VSS_E_INVALID_ARG, "null device pointer");
  int rc = check_frames(h, n, height, width, channels, row_stride, frame_stride, max_frames(h));
  if (rc) return rc;
  if (!rgba_geometry_ok(d_out_rgba, out_row_stride, out_frame_stride, height, width, false))
    return fail(h, VSS_E_INVALID_ARG, "bad RGBA output geometry (row stride >= 4*width, multiple of 4)");
  HIP_TRY(h, hipSetDevice(h->device));
  return composite_enqueue(h, d_frames, n, height, width, channels, row_stride, frame_stride, d_alpha_u8,
                           d_out_rgba, out_row_stride, out_frame_stride, stream_or(h, stream));
}

int vss_segment_composite(vss_handle* h, vss_post_state* st, const uint8_t* frames, int n, int height, int width,
                          int channels, size_t row_stride, uint8_t* out_rgba) {
  if (!h || !st || st->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / post state mismatch");
  if (!out_rgba) return fail(h, VSS_E_INVALID_ARG, "null output");
  std::lock_guard<std::mutex> pl(h->post_mu);
  std::unique_lock<std::mutex> lk(h->mu);
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t fs = row_stride * (size_t)height, ors = (size_t)width * 4, ofs = ors * height;
  int rc = comp_reserve(h, (size_t)n * ofs);
  if (rc) return rc;
  int k = 0;
  if ((rc = seam_on_stream(h, lk, frames, n, height, width, channels, row_stride, &k))) return rc;
  const Slot& s = h->slots[k];
  rc = post_enqueue(st, s.d_frames, n, height, width, channels, row_stride, fs, s.d_masks, nullptr, h->d_post_u8,
                    h->stream);
  if (!rc)
    rc = composite_enqueue(h, s.d_frames, n, height, width, channels, row_stride, fs, h->d_post_u8, h->d_comp, ors,
                           ofs, h->stream);
  return finish_seam(h, lk, k, comp_to_host(h, rc, out_rgba, (size_t)n * ofs));
}

}  // extern "C"

// ---- the post chain over many streams (vss_post.hip k_post_pool; include/vss_pool.h) ----
// p->mu held.  What a call may be refused for, before anything is enqueued.
int vss_engine::pool_check(vss_post_pool* p, const int* ids, int n, const uint8_t* d_frames, int fh, int fw, int fc, size_t rs,
               size_t fs, int max_n) {
  vss_handle* h = p->h;
  if (!ids) return fail(h, VSS_E_INVALID_ARG, "pool: null stream ids");
  if (!d_frames && p->cfg.use_bilateral) return fail(h, VSS_E_INVALID_ARG, "pool: null frames with use_bilateral on");
  if (int rc = check_frames(h, n, fh, fw, fc, rs, fs, max_n)) return rc;
  const uint64_t call = ++p->calls;
  for (int t = 0; t < n; ++t) {
    if (ids[t] < 0 || ids[t] >= p->capacity)
      return fail(h, VSS_E_INVALID_ARG, "pool: stream id " + std::to_string(ids[t]) + " outside [0, " +
                                            std::to_string(p->capacity) + ")");
    if (p->stamp[ids[t]] == call)
      return fail(h, VSS_E_INVALID_ARG, "pool: stream id " + std::to_string(ids[t]) + " twice in one call");
    p->stamp[ids[t]] = call;
  }
  return VSS_OK;
}

// p->mu held; arguments checked.  ceil(n / kPoolFrames) launches and the ordering event.
int vss_engine::pool_enqueue(vss_post_pool* p, const int* ids, int n, const uint8_t* d_frames, int fh, int fw, int fc, size_t rs,
                 size_t fs, const float* d_masks, const FaceFrame* d_faces, float* d_alpha, uint8_t* d_u8,
                 hipStream_t s) {
  vss_handle* h = p->h;
  const long P = (long)h->cfg.model_h * h->cfg.model_w;
  int rc = p->fence.wait_on(h, s);
  if (rc) return rc;
  PostPoolParams pp{};
  post_filter_params(&pp.f, h, p->cfg, p->tab, fh, fw, fc, rs, fs);
  pp.planes = p->planes;
  pp.a = p->cfg.ema;
  for (int t0 = 0; t0 < n && !rc; t0 += kPoolFrames) {
    const int m = std::min(kPoolFrames, n - t0);
    pp.f.faces = d_faces ? d_faces + t0 : nullptr;
    pp.f.frames = d_frames ? d_frames + (size_t)t0 * fs : nullptr;
    pp.f.alpha = d_alpha ? d_alpha + t0 * P : nullptr;
    pp.f.alpha_u8 = d_u8 ? d_u8 + t0 * P : nullptr;
    pp.masks = d_masks + t0 * P;
    for (int t = 0; t < m; ++t) {
      const int id = ids[t0 + t];
      pp.entry[t] = (unsigned)id << 2 | (unsigned)p->cur[id] << 1 | (unsigned)p->seen[id];
    }
    launch_post_pool(pp, m, s);
    rc = launched(h, "pool");
    // the launch is in the stream: these streams' prevAlpha is in their other plane from here on
    if (!rc)
      for (int t = 0; t < m; ++t) {
        const int id = ids[t0 + t];
        p->cur[id] ^= 1;
        p->seen[id] = 1;
      }
  }
  // also after a failed launch: what did go out reads and writes the planes
  const int rr = p->fence.record(h, s);
  return rr ? rr : rc;
}

extern "C" {

int vss_post_pool_create(vss_handle* h, const vss_post_config* cfg, int capacity, vss_post_pool** out) {
  if (!h || !out) return fail(h, VSS_E_INVALID_ARG, "null handle/out");
  *out = nullptr;
  if (capacity < 1 || capacity > (1 << 29)) return fail(h, VSS_E_INVALID_ARG, "pool: capacity must be in [1, 2^29]");
  if (h->cfg.model_h < 3 || h->cfg.model_w < 3) return fail(h, VSS_E_UNSUPPORTED, "mask too small for post");
  vss_post_config c;
  if (cfg) c = *cfg;
  else vss_post_config_default(&c);
  if (!(c.sigma_spatial > 0) || !(c.sigma_range > 0)) return fail(h, VSS_E_INVALID_ARG, "sigmas must be > 0");
  HIP_TRY(h, hipSetDevice(h->device));
  vss_post_pool* p = new vss_post_pool();
  p->h = h;
  p->cfg = c;
  p->capacity = capacity;
  p->seen.assign(capacity, 0);
  p->cur.assign(capacity, 0);
  p->stamp.assign(capacity, 0);
  const size_t P = (size_t)h->cfg.model_h * h->cfg.model_w;
  int rc = counted_alloc(h, &p->planes, &p->planes_bytes, (size_t)capacity * 2 * P * 4);
  if (!rc) rc = counted_alloc(h, &p->tab.rtab, &p->rtab_bytes, (size_t)kRangeTab * 8);
  if (!rc && p->fence.create() != hipSuccess) rc = fail(h, VSS_E_HIP, "pool: hipEventCreate failed");
  if (!rc && !p->tab.update(p->cfg)) rc = fail(h, VSS_E_HIP, "pool: table upload failed");
  if (rc) {
    vss_post_pool_destroy(p);
    return rc;
  }
  *out = p;
  return VSS_OK;
}

void vss_post_pool_destroy(vss_post_pool* p) {
  if (!p) return;
  (void)p->fence.quiesce(p->h);
  (void)counted_alloc(p->h, &p->planes, &p->planes_bytes, 0);
  (void)counted_alloc(p->h, &p->tab.rtab, &p->rtab_bytes, 0);
  p->fence.destroy();
  delete p;
}

int vss_post_pool_set_config(vss_post_pool* p, const vss_post_config* cfg) {
  if (!p) return fail(nullptr, VSS_E_INVALID_ARG, "null pool");
  if (!cfg) return fail(p->h, VSS_E_INVALID_ARG, "pool: null config");
  if (!(cfg->sigma_spatial > 0) || !(cfg->sigma_range > 0)) return fail(p->h, VSS_E_INVALID_ARG, "sigmas must be > 0");
  std::lock_guard<std::mutex> lk(p->mu);
  if (int rc = p->fence.quiesce(p->h)) return rc;  // the table may be rewritten: the pool's latest call has ended
  p->cfg = *cfg;
  if (!p->tab.update(p->cfg)) return fail(p->h, VSS_E_HIP, "pool: table upload failed");
  return VSS_OK;
}

int vss_post_pool_reset(vss_post_pool* p, int stream_id) {
  if (!p) return fail(nullptr, VSS_E_INVALID_ARG, "null pool");
  if (stream_id < -1 || stream_id >= p->capacity)
    return fail(p->h, VSS_E_INVALID_ARG, "pool: stream id " + std::to_string(stream_id) + " outside [0, " +
                                             std::to_string(p->capacity) + ") and not -1");
  std::lock_guard<std::mutex> lk(p->mu);
  // host state only: the stream's next frame is told that it is the first
  if (stream_id < 0) std::fill(p->seen.begin(), p->seen.end(), 0);
  else p->seen[stream_id] = 0;
  return VSS_OK;
}

int vss_post_pool_process_device(vss_post_pool* p, const int* stream_ids, int n, const uint8_t* d_frames, int height,
                                 int width, int channels, size_t row_stride, size_t frame_stride, const float* d_masks,
                                 const vss_face_frame* d_faces, float* d_alpha, uint8_t* d_alpha_u8, void* stream) {
  if (!p) return fail(nullptr, VSS_E_INVALID_ARG, "null pool");
  vss_handle* h = p->h;
  if (!d_masks) return fail(h, VSS_E_INVALID_ARG, "pool: null masks");
  std::lock_guard<std::mutex> lk(p->mu);
  int rc = pool_check(p, stream_ids, n, d_frames, height, width, channels, row_stride, frame_stride, max_frames(h));
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  return pool_enqueue(p, stream_ids, n, d_frames, height, width, channels, row_stride, frame_stride, d_masks,
                      reinterpret_cast<const FaceFrame*>(d_faces), d_alpha, d_alpha_u8, stream_or(h, stream));
}

int vss_segment_post_pool(vss_handle* h, vss_post_pool* p, const int* stream_ids, const uint8_t* frames, int n,
                          int height, int width, int channels, size_t row_stride, float* alpha_out,
                          uint8_t* alpha_u8_out) {
  if (!h || !p || p->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / post pool mismatch");
  if (!alpha_out && !alpha_u8_out) return fail(h, VSS_E_INVALID_ARG, "no output requested");
  if (!frames) return fail(h, VSS_E_INVALID_ARG, "null frames");
  std::lock_guard<std::mutex> pl(h->post_mu);
  std::lock_guard<std::mutex> ql(p->mu);
  int rc = pool_check(p, stream_ids, n, frames, height, width, channels, row_stride, row_stride * (size_t)height,
                      h->cfg.max_batch);
  if (rc) return rc;
  std::unique_lock<std::mutex> lk(h->mu);
  int k = 0;
  rc = seam_on_stream(h, lk, frames, n, height, width, channels, row_stride, &k);
  if (rc) return rc;
  const Slot& s = h->slots[k];
  const AlphaPlanes d = alpha_planes(h, alpha_out, alpha_u8_out);
  rc = pool_enqueue(p, stream_ids, n, s.d_frames, height, width, channels, row_stride, row_stride * (size_t)height,
                    s.d_masks, nullptr, d.f32, d.u8, h->stream);
  return finish_seam(h, lk, k, alpha_to_host(h, rc, n, alpha_out, alpha_u8_out));
}

}  // extern "C"
