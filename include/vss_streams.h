/* vss_streams.h — many streams to finished frames: one frame per stream in one
 * call, each over its own virtual background, from RGB(A) frames and alpha
 * bytes or from NV12 to NV12 (k_bg_streams_* in csrc/vss_background.hip,
 * k_matte_*_streams in csrc/vss_matte.hip).
 * Part of the C ABI of include/vss.h, which includes this header at its end;
 * include vss.h, not this file.
 *
 * Definition.  For every frame t, vss_background_composite_streams_device
 * writes, bit for bit, what
 *   vss_background_composite_device(h, bgs[t], frame t alone, n = 1, alpha t alone, ...)
 * writes — hence what the numpy restatements of that call give
 * (tests/background_ref.py, tests/layers_ref.py, tests/matte_ref.py).  The NV12
 * call writes pack(std, that composite over unpack(std, in)) with the alpha
 * bytes vss_post_pool_process_device produces for stream stream_ids[t] over
 * vss_segment_device on unpack(std, in); d_faces is forwarded to the pool
 * unchanged.
 *
 * All frames of a call share one geometry, as in the post pool.  bgs and
 * stream_ids are host arrays of n entries, not read after the call returns.
 * n is in 1..max_batch.  The same background object may stand for several
 * frames of a call (participants sharing a company plate): its caches — the
 * scaled image, the baked plate, the overlay plate — are shared by those frames,
 * and its per-frame scratch (k_blur_h's output, the matte's 17 B per mask
 * pixel) holds one slot per frame that names it, frame t using the slot of its
 * rank among them; the scratch is grown on demand and counted into
 * vss_info.device_bytes.  A steady loop whose shapes and settings do not change
 * allocates nothing, waits for nothing on the host and rebuilds no cache.
 *
 * The number of kernel launches of a call depends neither on n nor on the
 * number of distinct backgrounds (up to 32 frames per launch), except for the
 * one-off cache builds of an object whose image, layers or frame size changed.
 *
 * Ordering.  One call in flight per background object, as for
 * vss_background_composite_device: the call waits, on the device, for the
 * latest call of every distinct object it names, and every one of them is then
 * fenced by the event the call records after its launches (one record for the
 * call, which its objects share; also recorded when a launch failed, since
 * what did go out reads the objects' buffers).  The objects' locks are taken in
 * one fixed order, so concurrent calls that name the same objects in different
 * orders cannot deadlock.  Setters work between calls as they do today.
 *
 * VSS_E_INVALID_ARG (with a vss_last_error message) for a null pointer, an
 * object of another handle, n or a geometry out of range, a bgs[t] in image or
 * blur mode that was never given an image or a blur, refinement on for a bgs[t]
 * with a frame smaller than the mask, and whatever the post pool refuses (an id
 * out of range or twice).  Such a call enqueues nothing and moves no stream's
 * state: every background is checked before the pooled post chain is enqueued. */
#ifndef VSS_STREAMS_H_
#define VSS_STREAMS_H_

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frame t over bgs[t]; everything else as vss_background_composite_device. */
int vss_background_composite_streams_device(vss_handle* h, vss_background* const* bgs, int n,
                                            const uint8_t* d_frames, int height, int width, int channels,
                                            size_t row_stride, size_t frame_stride, const uint8_t* d_alpha_u8,
                                            uint8_t* d_out_rgba, size_t out_row_stride, size_t out_frame_stride,
                                            void* stream);

/* Host convenience, as vss_segment_background: the seam, the pooled post chain
 * and the per-stream backgrounds for one frame of each of n streams, tight RGBA
 * rows out; synchronous. */
int vss_segment_background_streams(vss_handle* h, vss_post_pool* p, const int* stream_ids,
                                   vss_background* const* bgs, const uint8_t* frames, int n, int height, int width,
                                   int channels, size_t row_stride, uint8_t* out_rgba);

/* NV12 in -> seam -> vss_post_pool (stream_ids) -> bgs[t] -> NV12 out, one frame
 * per stream, all enqueued on `stream` (NULL: the handle's), nothing waited
 * for.  d_faces: n vss_face_frame in device memory, or NULL.  The planes'
 * parameters are those of vss_video_process_device. */
int vss_video_process_streams_device(vss_video* v, vss_post_pool* p, const int* stream_ids,
                                     vss_background* const* bgs, const vss_face_frame* d_faces, const uint8_t* d_y,
                                     size_t y_pitch, size_t y_frame_stride, const uint8_t* d_uv, size_t uv_pitch,
                                     size_t uv_frame_stride, int n, int height, int width, uint8_t* d_out_y,
                                     size_t oy_pitch, size_t oy_frame_stride, uint8_t* d_out_uv, size_t ouv_pitch,
                                     size_t ouv_frame_stride, void* stream);

/* Host convenience: tightly packed host NV12 (y [n][h][w], uv [n][h/2][w]) in
 * and out; synchronous, as vss_video_process. */
int vss_video_process_streams(vss_video* v, vss_post_pool* p, const int* stream_ids, vss_background* const* bgs,
                              const uint8_t* y, const uint8_t* uv, int n, int height, int width, uint8_t* out_y,
                              uint8_t* out_uv);

#ifdef __cplusplus
}
#endif

#endif /* VSS_STREAMS_H_ */
