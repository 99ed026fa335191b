// vss_capi_streams.hip — the C ABI of many streams to finished frames
// (include/vss_streams.h): one frame per stream in one call, each over its own
// vss_background, over the engine in vss_capi.hip and the pool, background and
// video objects of the other units (vss_engine.h).
#include "vss_engine.h"

using namespace vss;
using namespace vss_engine;

namespace {

// The backgrounds' refusals, under their locks, before anything is enqueued.
// The locks are dropped again: the seam takes the handle's lock, which other
// calls hold while they take a background's.  The enqueue repeats the check
// under the locks it keeps, before the pool moves a stream.
int bgs_refusals(vss_handle* h, vss_background* const* bgs, int n, int fh, int fw) {
  BgStreamsLock bl(bgs, n);
  return bg_streams_check(h, bgs, n, fh, fw);
}

// p->mu held, pool_check and bgs_refusals passed, the seam's masks enqueued on
// s: the pooled post chain into d_alpha, then the composites.
int post_and_backgrounds(vss_handle* h, vss_post_pool* p, const int* ids, vss_background* const* bgs,
                         const FaceFrame* d_faces, const uint8_t* d_frames, int n, int fh, int fw, int fc, size_t rs,
                         size_t fs, const float* d_masks, uint8_t* d_alpha, uint8_t* d_out, size_t ors, size_t ofs,
                         hipStream_t s) {
  BgStreamsLock bl(bgs, n);
  int rc = bg_streams_check(h, bgs, n, fh, fw);  // a setter may have run since bgs_refusals
  if (!rc) rc = pool_enqueue(p, ids, n, d_frames, fh, fw, fc, rs, fs, d_masks, d_faces, nullptr, d_alpha, s);
  if (!rc) rc = bg_streams_enqueue(h, bl, bgs, n, d_frames, fh, fw, fc, rs, fs, d_alpha, d_out, ors, ofs, s);
  return rc;
}

int check_streams_call(vss_video* v, vss_post_pool* p) {
  if (!v) return fail(nullptr, VSS_E_INVALID_ARG, "null video");
  if (!p || p->h != v->h) return fail(v->h, VSS_E_INVALID_ARG, "video / post pool mismatch");
  return VSS_OK;
}

// v->mu and p->mu held; the planes' geometry checked.  What the ids and the
// backgrounds are refused for, before anything is enqueued.
int video_streams_refusals(vss_video* v, vss_post_pool* p, const int* ids, vss_background* const* bgs,
                           const uint8_t* d_y, int n, int fh, int fw) {
  vss_handle* h = v->h;
  const size_t rs = (size_t)fw * 4;
  int rc = bg_streams_args(h, bgs, n);
  if (!rc) rc = pool_check(p, ids, n, d_y, fh, fw, 4, rs, rs * fh, h->cfg.max_batch);
  if (!rc) rc = bgs_refusals(h, bgs, n, fh, fw);
  return rc;
}

// v->mu and p->mu held; video_streams_refusals passed.  The whole chain on s.
int video_streams_enqueue(vss_video* v, vss_post_pool* p, const int* ids, vss_background* const* bgs,
                          const FaceFrame* d_faces, const uint8_t* d_y, size_t yp, size_t yfs, const uint8_t* d_uv,
                          size_t up, size_t ufs, int n, int fh, int fw, uint8_t* d_oy, size_t oyp, size_t oyfs,
                          uint8_t* d_ouv, size_t oup, size_t oufs, hipStream_t s) {
  vss_handle* h = v->h;
  const size_t rs = (size_t)fw * 4, fs = rs * fh;
  int rc = video_reserve(v, n, fh, fw);
  if (rc) return rc;
  if ((rc = v->fence.wait_on(h, s))) return rc;
  const size_t P = (size_t)h->cfg.model_h * h->cfg.model_w, nb = (size_t)max_frames(h);
  uint8_t* d_in = v->d_buf;
  uint8_t* d_out = v->d_buf + v->px_cap * 4;
  float* d_masks = reinterpret_cast<float*>(v->d_buf + v->px_cap * 8);
  uint8_t* d_alpha = v->d_buf + v->px_cap * 8 + nb * P * 4;
  launch_nv12_unpack(nv12_params(v->std_, d_y, yp, yfs, d_uv, up, ufs, d_in, rs, fs, fh, fw), n, s);
  rc = launched(h, "nv12 unpack");
  if (!rc) rc = segment_device_on(h, &v->slot, d_in, n, fh, fw, 4, rs, fs, d_masks, s);
  if (!rc) rc = post_and_backgrounds(h, p, ids, bgs, d_faces, d_in, n, fh, fw, 4, rs, fs, d_masks, d_alpha, d_out, rs,
                                     fs, s);
  if (!rc) {
    launch_nv12_pack(nv12_params(v->std_, d_oy, oyp, oyfs, d_ouv, oup, oufs, d_out, rs, fs, fh, fw), n, s);
    rc = launched(h, "nv12 pack");
  }
  // also after a failed enqueue: what did go out reads or writes the scratch
  const int rr = v->fence.record(h, s);
  return rr ? rr : rc;
}

}  // namespace

extern "C" {

int vss_background_composite_streams_device(vss_handle* h, vss_background* const* bgs, int n,
                                            const uint8_t* d_frames, int height, int width, int channels,
                                            size_t row_stride, size_t frame_stride, const uint8_t* d_alpha_u8,
                                            uint8_t* d_out_rgba, size_t out_row_stride, size_t out_frame_stride,
                                            void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  if (!d_frames || !d_alpha_u8 || !d_out_rgba) return fail(h, VSS_E_INVALID_ARG, "null device pointer");
  int rc = check_frames(h, n, height, width, channels, row_stride, frame_stride, max_frames(h));
  if (rc) return rc;
  if (!rgba_geometry_ok(d_out_rgba, out_row_stride, out_frame_stride, height, width, false))
    return fail(h, VSS_E_INVALID_ARG, "bad RGBA output geometry (row stride >= 4*width, multiple of 4)");
  if ((rc = bg_streams_args(h, bgs, n))) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = stream_or(h, stream);
  BgStreamsLock bl(bgs, n);
  if ((rc = bg_streams_check(h, bgs, n, height, width))) return rc;
  return bg_streams_enqueue(h, bl, bgs, n, d_frames, height, width, channels, row_stride, frame_stride, d_alpha_u8,
                            d_out_rgba, out_row_stride, out_frame_stride, s);
}

int vss_segment_background_streams(vss_handle* h, vss_post_pool* p, const int* stream_ids,
                                   vss_background* const* bgs, const uint8_t* frames, int n, int height, int width,
                                   int channels, size_t row_stride, uint8_t* out_rgba) {
  if (!h || !p || p->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / post pool mismatch");
  if (!frames) return fail(h, VSS_E_INVALID_ARG, "null frames");
  if (!out_rgba) return fail(h, VSS_E_INVALID_ARG, "null output");
  std::lock_guard<std::mutex> pl(h->post_mu);
  std::lock_guard<std::mutex> ql(p->mu);
  const size_t fs = row_stride * (size_t)height, ors = (size_t)width * 4, ofs = ors * height;
  int rc = pool_check(p, stream_ids, n, frames, height, width, channels, row_stride, fs, h->cfg.max_batch);
  if (!rc) rc = bg_streams_args(h, bgs, n);
  if (!rc) rc = bgs_refusals(h, bgs, n, height, width);
  if (rc) return rc;
  std::unique_lock<std::mutex> lk(h->mu);
  HIP_TRY(h, hipSetDevice(h->device));
  if ((rc = comp_reserve(h, (size_t)n * ofs))) return rc;
  int k = 0;
  if ((rc = seam_on_stream(h, lk, frames, n, height, width, channels, row_stride, &k))) return rc;
  const Slot& s = h->slots[k];
  rc = post_and_backgrounds(h, p, stream_ids, bgs, nullptr, s.d_frames, n, height, width, channels, row_stride, fs,
                            s.d_masks, h->d_post_u8, h->d_comp, ors, ofs, h->stream);
  return finish_seam(h, lk, k, comp_to_host(h, rc, out_rgba, (size_t)n * ofs));
}

int vss_video_process_streams_device(vss_video* v, vss_post_pool* p, const int* stream_ids,
                                     vss_background* const* bgs, const vss_face_frame* d_faces, const uint8_t* d_y,
                                     size_t y_pitch, size_t y_frame_stride, const uint8_t* d_uv, size_t uv_pitch,
                                     size_t uv_frame_stride, int n, int height, int width, uint8_t* d_out_y,
                                     size_t oy_pitch, size_t oy_frame_stride, uint8_t* d_out_uv, size_t ouv_pitch,
                                     size_t ouv_frame_stride, void* stream) {
  int rc = check_streams_call(v, p);
  if (rc) return rc;
  vss_handle* h = v->h;
  rc = check_nv12(h, "input", d_y, y_pitch, y_frame_stride, d_uv, uv_pitch, uv_frame_stride, n, height, width,
                  h->cfg.max_batch);
  if (!rc)
    rc = check_nv12(h, "output", d_out_y, oy_pitch, oy_frame_stride, d_out_uv, ouv_pitch, ouv_frame_stride, n, height,
                    width, h->cfg.max_batch);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = stream_or(h, stream);
  std::lock_guard<std::mutex> lk(v->mu);
  std::lock_guard<std::mutex> ql(p->mu);
  if ((rc = video_streams_refusals(v, p, stream_ids, bgs, d_y, n, height, width))) return rc;
  return video_streams_enqueue(v, p, stream_ids, bgs, reinterpret_cast<const FaceFrame*>(d_faces), d_y, y_pitch,
                               y_frame_stride, d_uv, uv_pitch, uv_frame_stride, n, height, width, d_out_y, oy_pitch,
                               oy_frame_stride, d_out_uv, ouv_pitch, ouv_frame_stride, s);
}

int vss_video_process_streams(vss_video* v, vss_post_pool* p, const int* stream_ids, vss_background* const* bgs,
                              const uint8_t* y, const uint8_t* uv, int n, int height, int width, uint8_t* out_y,
                              uint8_t* out_uv) {
  int rc = check_streams_call(v, p);
  if (rc) return rc;
  vss_handle* h = v->h;
  const size_t w = width > 0 ? (size_t)width : 0, hh = height > 0 ? (size_t)height : 0;
  rc = check_nv12(h, "input", y, w, w * hh, uv, w, w * (hh / 2), n, height, width, h->cfg.max_batch);
  if (!rc) rc = check_nv12(h, "output", out_y, w, w * hh, out_uv, w, w * (hh / 2), n, height, width, h->cfg.max_batch);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(v->mu);
  std::lock_guard<std::mutex> ql(p->mu);
  if ((rc = video_streams_refusals(v, p, stream_ids, bgs, y, n, height, width))) return rc;
  const size_t yb = (size_t)n * w * hh, ub = yb / 2;  // bytes of the Y planes and of the UV planes
  if (2 * (yb + ub) > v->nv_bytes) {
    if ((rc = v->fence.quiesce(h))) return rc;
    if ((rc = counted_alloc(h, &v->d_nv, &v->nv_bytes, 2 * (yb + ub)))) return rc;
  }
  uint8_t* d_y = v->d_nv;
  uint8_t* d_uv = d_y + yb;
  uint8_t* d_oy = d_uv + ub;
  uint8_t* d_ouv = d_oy + yb;
  hipStream_t s = h->stream;
  if ((rc = v->fence.wait_on(h, s))) return rc;  // the planes' previous reader
  HIP_TRY(h, hipMemcpyAsync(d_y, y, yb, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_uv, uv, ub, hipMemcpyHostToDevice, s));
  rc = video_streams_enqueue(v, p, stream_ids, bgs, nullptr, d_y, w, w * hh, d_uv, w, w * (hh / 2), n, height, width,
                             d_oy, w, w * hh, d_ouv, w, w * (hh / 2), s);
  if (!rc) {
    HIP_TRY(h, hipMemcpyAsync(out_y, d_oy, yb, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_uv, d_ouv, ub, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipStreamSynchronize(s));
  return rc;
}

}  // extern "C"
