/* vss_pool.h — the post chain over many streams: one frame per stream in one
 * call (k_post_pool in csrc/vss_post.hip).
 * Part of the C ABI of include/vss.h, which includes this header at its end;
 * include vss.h, not this file.
 *
 * A vss_post_state holds one stream and its batch axis is time.  A pool holds
 * `capacity` streams, numbered 0 .. capacity-1, and its batch axis is streams:
 * frame t of a call is the NEXT frame of stream stream_ids[t].  For every
 * stream, the outputs over any interleaving of calls equal those of a dedicated
 * vss_post_state fed that stream's frames one at a time
 * (vss_postprocess_device with n = 1, after vss_post_set_faces_device for that
 * frame when d_faces is given).
 *
 * State: two mask planes per stream (the EMA is fused into the filter's tile
 * load; a neighbouring tile's halo and a warped tap read prevAlpha at pixels
 * another workgroup writes, so a call reads one plane and writes the other) and
 * one range table per pool: capacity * 2 * mask_h * mask_w * 4 bytes plus the
 * table, counted into vss_info.device_bytes.  Which plane is current and
 * whether a stream has seen a frame are kept on the host and passed to the
 * kernel by value, so no call and no reset waits for the device.
 *
 * One call in flight per pool, as for vss_background: the pool records an event
 * after each call, a call on another HIP stream than the previous one waits on
 * it on the device, and destroy and set_config wait for it on the host.
 * Destroy a pool before its handle. */
#ifndef VSS_POOL_H_
#define VSS_POOL_H_

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vss_post_pool vss_post_pool;

/* cfg NULL: the reference's defaults.  VSS_E_INVALID_ARG for capacity < 1. */
int vss_post_pool_create(vss_handle* h, const vss_post_config* cfg, int capacity, vss_post_pool** out);
void vss_post_pool_destroy(vss_post_pool* p);

/* Every stream of the pool, from the next call. */
int vss_post_pool_set_config(vss_post_pool* p, const vss_post_config* cfg);

/* stream_id's next frame is its first (-1: every stream's).  Does not wait for
 * the device: calls enqueued earlier are unaffected and may still be running. */
int vss_post_pool_reset(vss_post_pool* p, int stream_id);

/* As vss_postprocess_device, [n] indexing the call's streams: stream_ids = n
 * distinct ids in [0, capacity), host memory, not read after the call returns;
 * d_faces = n vss_face_frame in device memory, or NULL.  n in 1..max_batch.
 * VSS_E_INVALID_ARG (null pool, ids or masks; null frames with use_bilateral
 * on; n, an id or the frame geometry out of range; an id twice) enqueues
 * nothing and changes no stream's state. */
int vss_post_pool_process_device(vss_post_pool* p, const int* stream_ids, int n, const uint8_t* d_frames, int height,
                                 int width, int channels, size_t row_stride, size_t frame_stride, const float* d_masks,
                                 const vss_face_frame* d_faces, float* d_alpha, uint8_t* d_alpha_u8, void* stream);

/* Host-memory convenience, as vss_segment_post: the seam and the pooled chain
 * for one frame of each of n streams; synchronous.  Either output may be NULL,
 * not both. */
int vss_segment_post_pool(vss_handle* h, vss_post_pool* p, const int* stream_ids, const uint8_t* frames, int n,
                          int height, int width, int channels, size_t row_stride, float* alpha_out,
                          uint8_t* alpha_u8_out);

#ifdef __cplusplus
}
#endif

#endif /* VSS_POOL_H_ */
