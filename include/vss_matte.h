/* vss_matte.h — entry points of the edge-aware alpha (csrc/vss_matte.hip).
 * Part of the C ABI of include/vss.h, which includes this header at its end
 * and holds the definition of the refinement, step by step, in its comment on
 * the virtual backgrounds; include vss.h, not this file. */
#ifndef VSS_MATTE_H_
#define VSS_MATTE_H_

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* radius 0: refinement off (the default; eps ignored).  radius 1..
 * VSS_REFINE_MAX_RADIUS with eps in [1, 65025]: on, from the next composite,
 * in every mode.  VSS_E_INVALID_ARG otherwise, also for a NaN or infinite eps. */
int vss_background_set_refine(vss_background* bg, int radius, double eps);

/* The alpha vss_background_composite_device would blend with, alone:
 * d_out_alpha [n][height][width] u8, out_row_stride (>= width) and
 * out_frame_stride bytes apart.  Refinement on: A of step 7; off:
 * vss_composite_device's alpha.  Same arguments and in-flight rule otherwise. */
int vss_background_alpha_device(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int height,
                                int width, int channels, size_t row_stride, size_t frame_stride,
                                const uint8_t* d_alpha_u8, uint8_t* d_out_alpha, size_t out_row_stride,
                                size_t out_frame_stride, void* stream);
/* The same for alpha bytes [n][mask_h][mask_w] of any size >= 1 x 1, not only
 * the handle's model_h x model_w (which vss_create keeps to multiples of 16):
 * masks smaller than the refinement window, odd sizes. */
int vss_background_alpha_device_at(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int height,
                                   int width, int channels, size_t row_stride, size_t frame_stride,
                                   const uint8_t* d_alpha_u8, int mask_h, int mask_w, uint8_t* d_out_alpha,
                                   size_t out_row_stride, size_t out_frame_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VSS_MATTE_H_ */
