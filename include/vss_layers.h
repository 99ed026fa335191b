/* vss_layers.h — branding layers of the virtual backgrounds (csrc/vss_layers.hip).
 * Part of the C ABI of include/vss.h, which includes this header at its end;
 * include vss.h, not this file.
 *
 * The reference shows the person over a branded picture: updateCanvas
 * (client/customization.ts:35-78) draws the background image and then a
 * template of layers (client/data.json) — rounded translucent plates, a logo,
 * a QR code, icons, and the employee's name and contacts as text with a drop
 * shadow — each layer shown or hidden by a privacy level (:38-45).  Here the
 * layers are drawn into an overlay plate O on the GPU and O goes between the
 * background and the person, in every mode (colour, image, blur), so that
 * only finished frames leave the GPU.  A browser canvas is not reproducible;
 * what follows is a definition in exact integers (tests/layers_ref.py restates
 * it in numpy and the GPU matches it bit for bit).
 *
 * Canvas mapping.  Layers live on a design canvas canvas_w x canvas_h (the
 * reference: 1920 x 1080, :37).  A canvas coordinate v maps to a frame fh x fw
 * by
 *   map(v, canvas, frame) = floor((2*v*frame + canvas) / (2*canvas))
 * in 64-bit integers with true floor division (round half up, also for v < 0):
 * vss_layers_map.  A layer's destination rectangle is [X0, X1) x [Y0, Y1),
 * X0 = map(x, canvas_w, fw), X1 = map(x + width, canvas_w, fw), Y likewise with
 * canvas_h and fh: layers that abut on the canvas abut on the frame.  The
 * rectangle is clipped to the frame; an empty one draws nothing; x and y may
 * be negative or beyond the canvas (mapped coordinates are kept in 64 bits).
 *
 * Overlay plate.  O is premultiplied RGBA u8 [fh][fw] and starts at 0.  The
 * visible layers (privacy <= the object's level) are drawn in order by
 * premultiplied source-over, per channel including alpha:
 *   O' = min(255, S + (O*(255 - S.a) + 127) / 255)      (integer division)
 * S = the layer's premultiplied sample at that pixel, 0 outside its rectangle.
 *
 * VSS_LAYER_ROUNDED_RECT (ctx.roundRect + fill, :71-76): colour r, g, b, a (not
 * premultiplied) and a radius.
 *   R = min(map(radius, canvas_w, fw), (X1-X0)/2, (Y1-Y0)/2)   (as roundRect clamps)
 * Coverage n in 0..16 from 4 x 4 subsamples: in 1/8-pixel units, sample (i, j)
 * of pixel (x, y) is (8x + 2i + 1, 8y + 2j + 1).  A sample counts if it lies
 * inside the rectangle and, where it falls into one of the four R x R corner
 * squares, dx^2 + dy^2 <= (8R)^2 from that corner's centre (the square's inner
 * vertex).  S.a = (a*n + 8) >> 4, S.c = (c*S.a + 127) / 255.  R = 0: a plain
 * rectangle, n = 16 everywhere inside.
 *
 * VSS_LAYER_IMAGE (ctx.drawImage, :67-70): a host RGBA u8 sprite
 * [src_h][src_w][4], row_stride bytes per row.  It is premultiplied once at
 * upload, c' = (c*a + 127) / 255; each of the four premultiplied channels is
 * scaled to (Y1-Y0) x (X1-X0) with VSS_BG_IMAGE's recipe (the half-pixel taps,
 * three f32 fma lerps, rounded half up), then c = min(c, a).  The scaling's
 * coordinates are relative to the unclipped rectangle.
 *
 * Drop shadow (ctx.shadow*, :53-58).  Either type may carry one: colour
 * r, g, b, a, a blur, dx, dy.  It is drawn immediately before its layer:
 *  1. P = the layer's sampled alpha S.a, drawn at the rectangle shifted by
 *     (map(dx, canvas_w, fw), map(dy, canvas_h, fh)); 0 elsewhere and outside
 *     the frame.
 *  2. sigma = blur * fw / (2.0 * canvas_w) in doubles (the canvas's standard
 *     deviation is half the blur; the horizontal scale serves both axes).
 *  3. r = min(32, (int)ceil(3*sigma)).
 *  4. r < 1, or vss_blur_weights(r, sigma) refuses: B = P.
 *  5. Otherwise B = the separable blur of P with those weights, zero padding,
 *     the horizontal pass then the vertical one, each (sum w*v + 32768) >> 16
 *     stored as u8.
 *  6. The shadow's sample: a_s = (a*B + 127) / 255, c_s = (c*a_s + 127) / 255.
 *
 * Background under the person.  In every mode
 *   bg' = min(255, O.c + (bg.c*(255 - O.a) + 127) / 255)
 * and the blend out = (fg*A + bg'*(255-A) + 127) / 255 of vss.h runs unchanged.
 * With no visible layer O = 0 and bg' = bg.  Colour and image backgrounds are
 * static: bg' is baked once into the cached frame-size plate, and layers cost
 * nothing per frame.  In blur mode O is read per frame (4 B per pixel).
 *
 * Text.  There is no font engine here: text is a VSS_LAYER_IMAGE whose sprite
 * the host rasterises (the Python helper template_layers maps the reference's
 * templates to layers around a caller-supplied rasteriser).
 *
 * O is rebuilt by the first composite after the layers, the level or the frame
 * size change, on that composite's stream. */
#ifndef VSS_LAYERS_H_
#define VSS_LAYERS_H_

#include "vss.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { VSS_LAYER_IMAGE = 0, VSS_LAYER_ROUNDED_RECT = 1 };
#define VSS_MAX_LAYERS 32
#define VSS_LAYER_MAX_SPRITE 4096 /* a sprite's larger side */

typedef struct vss_layer {
  int type;               /* VSS_LAYER_IMAGE / VSS_LAYER_ROUNDED_RECT */
  int privacy;            /* 1 (low) .. 3 (high): drawn when <= the object's level */
  int x, y;               /* canvas coordinates; may be negative or beyond the canvas */
  int width, height;      /* >= 0 */
  int radius;             /* ROUNDED_RECT: >= 0, canvas units */
  uint8_t color[4];       /* ROUNDED_RECT: r, g, b, a, not premultiplied */
  const uint8_t* pixels;  /* IMAGE: host RGBA u8 [src_h][src_w][4], not premultiplied */
  int src_h, src_w;       /* IMAGE: 1 .. VSS_LAYER_MAX_SPRITE */
  size_t row_stride;      /* IMAGE: bytes per sprite row, >= 4 * src_w */
  int has_shadow;         /* 0: none (the shadow fields are ignored) */
  uint8_t shadow_color[4];
  int shadow_blur;        /* >= 0, canvas units (ctx.shadowBlur) */
  int shadow_dx, shadow_dy;
} vss_layer;

/* map(v, canvas, frame) above; host-only, no GPU needed.  canvas < 1: 0. */
int vss_layers_map(int v, int canvas, int frame);

/* Replaces the object's layers by layers[0 .. n) on a canvas_w x canvas_h canvas.
 * Every sprite is copied to the GPU before the call returns; the host pointers
 * are not read afterwards.  n = 0 removes the layers and releases their memory
 * (layers may be null, the canvas size must still be >= 1).
 * VSS_E_INVALID_ARG, with a message and no state changed: n outside
 * 0..VSS_MAX_LAYERS; a canvas size < 1; a null array with n > 0; an unknown
 * type; a privacy outside 1..3; width, height, radius or shadow_blur < 0; a
 * null sprite, a sprite side outside 1..VSS_LAYER_MAX_SPRITE or a row stride
 * below 4 * src_w. */
int vss_background_set_layers(vss_background* bg, const vss_layer* layers, int n, int canvas_w, int canvas_h);

/* The privacy level, 1..3: layers with privacy <= level are drawn.  2 after
 * create (customization.ts:28). */
int vss_background_set_privacy(vss_background* bg, int level);

/* The plate O alone for a frame height x width: d_out [height][width][4]
 * premultiplied RGBA, row_stride (>= 4 * width) bytes per row, enqueued on `stream` (null: the handle's).  For tests and for hosts
 * that composite themselves.  VSS_E_INVALID_ARG when bg belongs to another
 * handle, for a height or width outside 1..16384 or a row stride below
 * 4 * width.  Same in-flight rule as the composites. */
int vss_background_overlay_device(vss_handle* h, vss_background* bg, int height, int width, uint8_t* d_out,
                                  size_t row_stride, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VSS_LAYERS_H_ */
