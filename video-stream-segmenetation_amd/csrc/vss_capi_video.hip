// vss_capi_video.hip — the C ABI of NV12 video I/O (vss_video.hip; the
// definition: include/vss_video.h), over the engine in vss_capi.hip and the
// post state and background of the other units (vss_engine.h).
#include "vss_engine.h"

using namespace vss;
using namespace vss_engine;

namespace {

constexpr CscCoef kCsc[4] = {
    {16, 298, 409, -100, -208, 516, 66, 129, 25, -38, -74, 112, 112, -94, -18},    // BT.601 limited
    {16, 298, 459, -55, -136, 541, 47, 157, 16, -26, -86, 112, 112, -102, -10},    // BT.709 limited
    {0, 256, 359, -88, -183, 454, 77, 150, 29, -43, -85, 128, 128, -107, -21},     // BT.601 full
    {0, 256, 403, -48, -120, 475, 54, 183, 19, -29, -99, 128, 128, -116, -12},     // BT.709 full
};

int check_std(vss_handle* h, int std) {
  if (std < 0 || std > 3) return fail(h, VSS_E_INVALID_ARG, "std must be one of VSS_CSC_* (0..3)");
  return VSS_OK;
}

}  // namespace

// one NV12 batch's geometry; `what` names the planes in the message
int vss_engine::check_nv12(vss_handle* h, const char* what, const uint8_t* y, size_t yp, size_t yfs, const uint8_t* uv, size_t up,
               size_t ufs, int n, int fh, int fw, int max_n) {
  const std::string w(what);
  if (!y || !uv) return fail(h, VSS_E_INVALID_ARG, w + ": null plane pointer");
  if (n < 1 || n > max_n) return fail(h, VSS_E_INVALID_ARG, "n must be in [1, max_batch]");
  if (fh < 2 || fw < 2 || (fh & 1) || (fw & 1))
    return fail(h, VSS_E_INVALID_ARG, "NV12 needs an even height and width, both >= 2");
  if (yp < (size_t)fw || up < (size_t)fw) return fail(h, VSS_E_INVALID_ARG, w + ": pitch < width");
  if (yfs < yp * (size_t)fh) return fail(h, VSS_E_INVALID_ARG, w + ": y_frame_stride < y_pitch * height");
  if (ufs < up * (size_t)(fh / 2)) return fail(h, VSS_E_INVALID_ARG, w + ": uv_frame_stride < uv_pitch * height/2");
  return VSS_OK;
}

namespace {

int check_rgba(vss_handle* h, const uint8_t* p, size_t rs, size_t fs, int fh, int fw) {
  if (!p) return fail(h, VSS_E_INVALID_ARG, "null RGBA pointer");
  if (!rgba_geometry_ok(p, rs, fs, fh, fw, true))
    return fail(h, VSS_E_INVALID_ARG,
                "bad RGBA geometry (row stride >= 4*width; strides and base pointer multiples of 4)");
  return VSS_OK;
}

}  // namespace

Nv12Params vss_engine::nv12_params(int std, const uint8_t* y, size_t yp, size_t yfs, const uint8_t* uv, size_t up, size_t ufs,
                       const uint8_t* rgba, size_t rs, size_t fs, int fh, int fw) {
  Nv12Params p{};
  p.y = const_cast<uint8_t*>(y);
  p.uv = const_cast<uint8_t*>(uv);
  p.y_pitch = (long)yp; p.y_frame_stride = (long)yfs;
  p.uv_pitch = (long)up; p.uv_frame_stride = (long)ufs;
  p.rgba = const_cast<uint8_t*>(rgba);
  p.row_stride = (long)rs; p.frame_stride = (long)fs;
  p.fh = fh; p.fw = fw;
  p.k = kCsc[std];
  return p;
}

// v->mu held: the scratch for n frames fh x fw
int vss_engine::video_reserve(vss_video* v, int n, int fh, int fw) {
  vss_handle* h = v->h;
  const size_t px = (size_t)n * fh * fw, P = (size_t)h->cfg.model_h * h->cfg.model_w;
  const size_t nb = (size_t)max_frames(h);
  if (px <= v->px_cap) return VSS_OK;
  int rc = v->fence.quiesce(h);  // the scratch is freed: v's latest call has ended
  if (rc) return rc;
  v->px_cap = 0;
  if ((rc = counted_alloc(h, &v->d_buf, &v->buf_bytes, px * 8 + nb * P * 5))) return rc;
  v->px_cap = px;
  return VSS_OK;
}

namespace {

// v->mu held; arguments checked.  The whole chain on s.
int video_enqueue(vss_video* v, vss_post_state* st, vss_background* bg, const uint8_t* d_y, size_t yp, size_t yfs,
                  const uint8_t* d_uv, size_t up, size_t ufs, int n, int fh, int fw, uint8_t* d_oy, size_t oyp,
                  size_t oyfs, uint8_t* d_ouv, size_t oup, size_t oufs, hipStream_t s) {
  vss_handle* h = v->h;
  const size_t P = (size_t)h->cfg.model_h * h->cfg.model_w, nb = (size_t)max_frames(h);
  int rc = video_reserve(v, n, fh, fw);
  if (rc) return rc;
  if ((rc = v->fence.wait_on(h, s))) return rc;
  uint8_t* d_in = v->d_buf;
  uint8_t* d_out = v->d_buf + v->px_cap * 4;
  float* d_masks = reinterpret_cast<float*>(v->d_buf + v->px_cap * 8);
  uint8_t* d_alpha = v->d_buf + v->px_cap * 8 + nb * P * 4;
  const size_t rs = (size_t)fw * 4, fs = rs * fh;
  launch_nv12_unpack(nv12_params(v->std_, d_y, yp, yfs, d_uv, up, ufs, d_in, rs, fs, fh, fw), n, s);
  rc = launched(h, "nv12 unpack");
  if (!rc) rc = segment_device_on(h, &v->slot, d_in, n, fh, fw, 4, rs, fs, d_masks, s);
  if (!rc) rc = vss_postprocess_device(st, d_in, n, fh, fw, 4, rs, fs, d_masks, nullptr, d_alpha, s);
  if (!rc) {
    std::lock_guard<std::mutex> bl(bg->mu);
    rc = bg_enqueue(h, bg, d_in, n, fh, fw, 4, rs, fs, d_alpha, d_out, rs, fs, s);
  }
  if (!rc) {
    launch_nv12_pack(nv12_params(v->std_, d_oy, oyp, oyfs, d_ouv, oup, oufs, d_out, rs, fs, fh, fw), n, s);
    rc = launched(h, "nv12 pack");
  }
  // also after a failed enqueue: what did go out reads or writes the scratch
  const int rr = v->fence.record(h, s);
  return rr ? rr : rc;
}

int check_video_call(vss_video* v, vss_post_state* st, vss_background* bg) {
  if (!v) return fail(nullptr, VSS_E_INVALID_ARG, "null video");
  if (!st || st->h != v->h) return fail(v->h, VSS_E_INVALID_ARG, "video / post state mismatch");
  if (!bg || bg->h != v->h) return fail(v->h, VSS_E_INVALID_ARG, "video / background mismatch");
  return VSS_OK;
}

}  // namespace

static_assert(VSS_CSC_BT601_LIMITED == 0 && VSS_CSC_BT709_LIMITED == 1 && VSS_CSC_BT601_FULL == 2 &&
                  VSS_CSC_BT709_FULL == 3,
              "kCsc is indexed by VSS_CSC_*");

extern "C" {

int vss_nv12_to_rgba_device(vss_handle* h, int std, const uint8_t* d_y, size_t y_pitch, size_t y_frame_stride,
                            const uint8_t* d_uv, size_t uv_pitch, size_t uv_frame_stride, int n, int height, int width,
                            uint8_t* d_rgba, size_t row_stride, size_t frame_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  int rc = check_std(h, std);
  if (!rc)
    rc = check_nv12(h, "input", d_y, y_pitch, y_frame_stride, d_uv, uv_pitch, uv_frame_stride, n, height, width,
                    max_frames(h));
  if (!rc) rc = check_rgba(h, d_rgba, row_stride, frame_stride, height, width);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  launch_nv12_unpack(nv12_params(std, d_y, y_pitch, y_frame_stride, d_uv, uv_pitch, uv_frame_stride, d_rgba, row_stride,
                                 frame_stride, height, width), n, stream_or(h, stream));
  return launched(h, "nv12 unpack");
}

int vss_rgba_to_nv12_device(vss_handle* h, int std, const uint8_t* d_rgba, size_t row_stride, size_t frame_stride,
                            int n, int height, int width, uint8_t* d_y, size_t y_pitch, size_t y_frame_stride,
                            uint8_t* d_uv, size_t uv_pitch, size_t uv_frame_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  int rc = check_std(h, std);
  if (!rc)
    rc = check_nv12(h, "output", d_y, y_pitch, y_frame_stride, d_uv, uv_pitch, uv_frame_stride, n, height, width,
                    max_frames(h));
  if (!rc) rc = check_rgba(h, d_rgba, row_stride, frame_stride, height, width);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  launch_nv12_pack(nv12_params(std, d_y, y_pitch, y_frame_stride, d_uv, uv_pitch, uv_frame_stride, d_rgba, row_stride,
                               frame_stride, height, width), n, stream_or(h, stream));
  return launched(h, "nv12 pack");
}

int vss_video_create(vss_handle* h, int std, vss_video** out) {
  if (!h || !out) return fail(h, VSS_E_INVALID_ARG, "null handle/out");
  *out = nullptr;
  if (int rc = check_std(h, std)) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  vss_video* v = new vss_video();
  v->h = h;
  v->std_ = std;
  const hipError_t e = v->fence.create();
  if (e != hipSuccess) {
    delete v;
    return fail(h, VSS_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
  }
  *out = v;
  return VSS_OK;
}

void vss_video_destroy(vss_video* v) {
  if (!v) return;
  (void)v->fence.quiesce(v->h);
  (void)counted_alloc(v->h, &v->d_buf, &v->buf_bytes, 0);
  (void)counted_alloc(v->h, &v->d_nv, &v->nv_bytes, 0);
  v->fence.destroy();
  delete v;
}

int vss_video_set_standard(vss_video* v, int std) {
  if (!v) return fail(nullptr, VSS_E_INVALID_ARG, "null video");
  if (int rc = check_std(v->h, std)) return rc;
  std::lock_guard<std::mutex> lk(v->mu);
  v->std_ = std;
  return VSS_OK;
}

int vss_video_process_device(vss_video* v, vss_post_state* st, vss_background* bg, const uint8_t* d_y, size_t y_pitch,
                             size_t y_frame_stride, const uint8_t* d_uv, size_t uv_pitch, size_t uv_frame_stride, int n,
                             int height, int width, uint8_t* d_out_y, size_t oy_pitch, size_t oy_frame_stride,
                             uint8_t* d_out_uv, size_t ouv_pitch, size_t ouv_frame_stride, void* stream) {
  int rc = check_video_call(v, st, bg);
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
  return video_enqueue(v, st, bg, d_y, y_pitch, y_frame_stride, d_uv, uv_pitch, uv_frame_stride, n, height, width,
                       d_out_y, oy_pitch, oy_frame_stride, d_out_uv, ouv_pitch, ouv_frame_stride, s);
}

int vss_video_process(vss_video* v, vss_post_state* st, vss_background* bg, const uint8_t* y, const uint8_t* uv, int n,
                      int height, int width, uint8_t* out_y, uint8_t* out_uv) {
  int rc = check_video_call(v, st, bg);
  if (rc) return rc;
  vss_handle* h = v->h;
  const size_t w = width > 0 ? (size_t)width : 0, hh = height > 0 ? (size_t)height : 0;
  rc = check_nv12(h, "input", y, w, w * hh, uv, w, w * (hh / 2), n, height, width, h->cfg.max_batch);
  if (!rc) rc = check_nv12(h, "output", out_y, w, w * hh, out_uv, w, w * (hh / 2), n, height, width, h->cfg.max_batch);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(v->mu);
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
  rc = video_enqueue(v, st, bg, d_y, w, w * hh, d_uv, w, w * (hh / 2), n, height, width, d_oy, w, w * hh, d_ouv, w,
                     w * (hh / 2), s);
  if (!rc) {
    HIP_TRY(h, hipMemcpyAsync(out_y, d_oy, yb, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(out_uv, d_ouv, ub, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipStreamSynchronize(s));
  return rc;
}

}  // extern "C"
