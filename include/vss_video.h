/* vss_video.h — NV12 video I/O (csrc/vss_video.hip): colour conversion between
 * a decoder's / encoder's NV12 frames and the library's packed RGBA, and the
 * one-call device path NV12 in -> seam -> post chain -> background -> NV12 out.
 * Part of the C ABI of include/vss.h, which includes this header at its end;
 * include vss.h, not this file.
 *
 * NV12 frame layout.  A frame of height fh and width fw (both even, >= 2) is
 *   Y  [fh][y_pitch]     u8, one luma byte per pixel, and
 *   UV [fh/2][uv_pitch]  u8, fw/2 interleaved (U, V) pairs per row: the pair of
 *                        the 2x2 pixel block (y/2, x/2) at UV[y/2][2*(x/2)].
 * The two planes are separate device pointers; frame t's planes start
 * t * y_frame_stride and t * uv_frame_stride bytes after frame 0's.
 * y_pitch >= fw, uv_pitch >= fw, y_frame_stride >= y_pitch * fh and
 * uv_frame_stride >= uv_pitch * fh/2.  No alignment is required of pitches or
 * base pointers; bytes between fw and the pitch are never written.  RGBA
 * frames are as everywhere in vss.h: 4 bytes per pixel, row stride >= 4*width;
 * here the row stride, the frame stride and the base pointer are multiples of 4.
 *
 * The conversion.  All arithmetic is in 32-bit signed integers, `>> 8` is the
 * floor division by 256 and clip clamps to 0..255.  Per standard:
 *
 *   std            y0   cy   rv    gu    gv   bu   Y(r,g,b)      U(r,g,b)        V(r,g,b)
 *   BT601_LIMITED  16  298  409  -100  -208  516   66 129  25   -38  -74  112   112  -94  -18
 *   BT709_LIMITED  16  298  459   -55  -136  541   47 157  16   -26  -86  112   112 -102  -10
 *   BT601_FULL      0  256  359   -88  -183  454   77 150  29   -43  -85  128   128 -107  -21
 *   BT709_FULL      0  256  403   -48  -120  475   54 183  19   -29  -99  128   128 -116  -12
 *
 * Unpack (NV12 -> RGBA): pixel (y, x) takes Y[y][x] and the (U, V) pair of its
 * 2x2 block, replicated over the block (no interpolation).  With
 * c = cy*(Y - y0), d = U - 128, e = V - 128:
 *   R = clip((c + rv*e + 128) >> 8)
 *   G = clip((c + gu*d + gv*e + 128) >> 8)
 *   B = clip((c + bu*d + 128) >> 8)
 *   A = 255
 * Pack (RGBA -> NV12): per pixel
 *   Y = clip(((Yr*R + Yg*G + Yb*B + 128) >> 8) + y0);
 * per 2x2 block and channel the rounded mean m = (p00 + p01 + p10 + p11 + 2) >> 2
 * of the four pixels, then
 *   U = clip(((Ur*mR + Ug*mG + Ub*mB + 128) >> 8) + 128),  V likewise.
 * The input alpha byte is ignored.  (The full-range standards reach 256 before
 * the clamp: pure blue gives U = 256.)
 *
 * tests/video_ref.py restates this in numpy; the GPU matches it bit for bit. */
#ifndef VSS_VIDEO_H_
#define VSS_VIDEO_H_

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSS_CSC_BT601_LIMITED 0
#define VSS_CSC_BT709_LIMITED 1
#define VSS_CSC_BT601_FULL 2
#define VSS_CSC_BT709_FULL 3

/* Every call below returns VSS_E_INVALID_ARG, with a vss_last_error message
 * and nothing enqueued or written, for: an odd or sub-2 width or height, a
 * pitch below width, a frame stride below pitch * rows, std outside 0..3, a
 * null pointer, n above the handle's max_batch, and an object of another handle. */

/* The conversions alone, enqueued on `stream` (NULL: the handle's stream),
 * nothing waited for. */
int vss_nv12_to_rgba_device(vss_handle* h, int std, const uint8_t* d_y, size_t y_pitch, size_t y_frame_stride,
                            const uint8_t* d_uv, size_t uv_pitch, size_t uv_frame_stride, int n, int height, int width,
                            uint8_t* d_rgba, size_t row_stride, size_t frame_stride, void* stream);
int vss_rgba_to_nv12_device(vss_handle* h, int std, const uint8_t* d_rgba, size_t row_stride, size_t frame_stride,
                            int n, int height, int width, uint8_t* d_y, size_t y_pitch, size_t y_frame_stride,
                            uint8_t* d_uv, size_t uv_pitch, size_t uv_frame_stride, void* stream);

/* A vss_video owns the scratch of the one-call path: the unpacked RGBA frames,
 * the composited RGBA frames, the masks and the alpha bytes (and, for the host
 * call, the NV12 device planes).  Sized on first use, grown when
 * n * height * width grows, counted into vss_info.device_bytes, released on
 * destroy.  While the shape stays the same the scratch addresses do too, and
 * the object keeps to one of the handle's slots, so a steady loop replays that
 * slot's executable graph: no build and no patch after a shape's first call.
 * One call is in flight per object, as for vss_background: a call on another
 * stream is ordered after the previous one, and a call that regrows the
 * scratch waits for it on the host.  Destroy before vss_destroy. */
typedef struct vss_video vss_video;
int  vss_video_create(vss_handle* h, int std, vss_video** out);   /* INVALID_ARG: std outside 0..3 */
void vss_video_destroy(vss_video* v);
int  vss_video_set_standard(vss_video* v, int std);   /* from the next call */

/* NV12 in -> seam -> post chain -> background -> NV12 out, all enqueued on
 * `stream`, nothing waited for.  The output equals, bit for bit,
 *   pack(std, vss_background_composite_device(unpack(std, in), alpha))
 * with alpha the u8 alpha of vss_postprocess_device (st) over
 * vss_segment_device on unpack(std, in).  The background's mode and its
 * refinement apply unchanged: they see the unpacked RGBA. */
int vss_video_process_device(vss_video* v, vss_post_state* st, vss_background* bg, const uint8_t* d_y, size_t y_pitch,
                             size_t y_frame_stride, const uint8_t* d_uv, size_t uv_pitch, size_t uv_frame_stride, int n,
                             int height, int width, uint8_t* d_out_y, size_t oy_pitch, size_t oy_frame_stride,
                             uint8_t* d_out_uv, size_t ouv_pitch, size_t ouv_frame_stride, void* stream);

/* Host convenience: tightly packed host NV12 (y [n][h][w], uv [n][h/2][w]) in and out; synchronous. */
int vss_video_process(vss_video* v, vss_post_state* st, vss_background* bg, const uint8_t* y, const uint8_t* uv, int n,
                      int height, int width, uint8_t* out_y, uint8_t* out_uv);

#ifdef __cplusplus
}
#endif

#endif /* VSS_VIDEO_H_ */
