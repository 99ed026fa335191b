// vss_capi_background.hip — the C ABI of the virtual backgrounds
// (vss_background.hip), the edge-aware matte (vss_matte.hip, include/vss_matte.h)
// and the branding layers (vss_layers.hip, include/vss_layers.h), over the
// engine in vss_capi.hip (vss_engine.h).
#include <climits>
#include <cmath>

#include "vss_engine.h"

using namespace vss;
using namespace vss_engine;

namespace {

// w[0..2r]: 16-bit fixed-point Gaussian taps that sum to 65536 exactly
int blur_weights(int radius, double sigma, uint16_t* w, std::string* why) {
  if (radius < 1 || radius > kBlurMaxRadius) {
    *why = "blur radius must be in [1, 32]";
    return VSS_E_INVALID_ARG;
  }
  if (!(sigma > 0.0) || std::isinf(sigma)) {
    *why = "blur sigma must be a finite number > 0";
    return VSS_E_INVALID_ARG;
  }
  double g[2 * kBlurMaxRadius + 1], sum = 0.0;
  for (int k = -radius; k <= radius; ++k) sum += g[k + radius] = std::exp(-(double)(k * k) / (2.0 * sigma * sigma));
  long rest = 0;
  for (int k = 0; k <= 2 * radius; ++k) {
    if (k == radius) continue;
    const long v = (long)std::floor(65536.0 * g[k] / sum + 0.5);
    w[k] = (uint16_t)v;
    rest += v;
  }
  if (rest == 0) {  // the centre tap would be 65536: no u16, and no blur
    *why = "blur sigma too small: every off-centre 16-bit weight rounds to 0";
    return VSS_E_INVALID_ARG;
  }
  // The centre takes what the rounded taps leave.  With a wide sigma the 2r
  // rounding errors can add up to more than the table's own slope at the
  // centre (radius 32, sigma 40: 1116 left between two taps of 1120), and the
  // kernel would dip at its peak.  Then the m innermost tap pairs give one
  // unit each to the centre, m the smallest count that leaves the table
  // non-increasing from the centre outwards; no tap moves by more than 1.
  long centre = 65536 - rest;
  if (centre < w[radius + 1]) {
    const long first = w[radius + 1];
    int m = 0;
    for (int k = 1; k <= radius && !m; ++k)
      if (centre + 2 * k >= first - 1 && (k == radius || w[radius + k] - 1 >= w[radius + k + 1])) m = k;
    for (int k = 1; k <= m; ++k) {
      --w[radius + k];
      --w[radius - k];
    }
    centre += 2 * m;
  }
  w[radius] = (uint16_t)centre;
  return VSS_OK;
}

// bg->mu held.  One device buffer of bg holds `need` bytes; it grows only once
// bg's latest composite, which may still use it, has ended.
template <class T>
int bg_grow(vss_background* bg, T** p, size_t* have, size_t need) {
  if (need <= *have) return VSS_OK;
  const int rc = bg->fence.quiesce(bg->h);
  return rc ? rc : counted_alloc(bg->h, p, have, need);
}

// bg->mu held.  The matte's mask-resolution stage for these frames (refinement
// on): *ab = the (abar, bbar) plane the frame-resolution kernels apply.
int matte_enqueue(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int fh, int fw, int fc, size_t rs,
                  size_t fs, const uint8_t* d_alpha, int H, int W, hipStream_t s, const float2** ab) {
  if (fh < H || fw < W)
    return fail(h, VSS_E_INVALID_ARG, "refinement needs a frame no smaller than the mask (" + std::to_string(H) +
                                          " x " + std::to_string(W) + "); turn it off for smaller frames");
  if (W > 16384) return fail(h, VSS_E_INVALID_ARG, "refinement: mask wider than 16384");
  const size_t px = (size_t)n * H * W, need = px * 17;  // float2 + int2 + u8 per mask pixel
  if (int rc = bg_grow(bg, &bg->d_matte, &bg->matte_bytes, need)) return rc;
  MatteParams m{};
  m.frames = d_frames;
  m.row_stride = (long)rs;
  m.frame_stride = (long)fs;
  m.fh = fh; m.fw = fw; m.fc = fc;
  m.alpha = d_alpha;
  m.H = H; m.W = W;
  m.radius = bg->refine_radius;
  m.eps = bg->refine_eps;
  m.ab = reinterpret_cast<float2*>(bg->d_matte);
  m.q = reinterpret_cast<int2*>(bg->d_matte + px * 8);
  m.L = bg->d_matte + px * 16;
  launch_matte_stage(m, n, s);
  *ab = m.ab;
  return VSS_OK;
}

// map(v, canvas, frame) of include/vss_layers.h: round half up with true floor division
long layers_map(long v, long canvas, long frame) {
  const long num = 2 * v * frame + canvas, den = 2 * canvas;
  long q = num / den;
  if (num % den < 0) --q;
  return q;
}

bool layers_visible(const vss_background* bg) {
  for (const auto& L : bg->layers)
    if (L.l.privacy <= bg->level) return true;
  return false;
}

int clip(long v, int hi) { return (int)std::min<long>(std::max<long>(v, 0), hi); }

// bg->mu held; some layer is visible.  The overlay plate O for a frame fh x fw,
// rebuilt on s when the layers, the level or the frame size changed.
int plate_enqueue(vss_handle* h, vss_background* bg, int fh, int fw, hipStream_t s) {
  if (bg->plate_fh == fh && bg->plate_fw == fw) return VSS_OK;
  const int pitch = layer_pitch(fw);
  const size_t need = (size_t)pitch * fh * 4;
  bool shadows = false;
  for (const auto& L : bg->layers) shadows |= L.l.privacy <= bg->level && L.l.has_shadow;
  const size_t need_sh = shadows ? (size_t)pitch * fh * 2 : 0;
  int rc = bg_grow(bg, &bg->d_plate, &bg->plate_bytes, need);
  if (!rc) rc = bg_grow(bg, &bg->d_shadow, &bg->shadow_bytes, need_sh);
  if (rc) return rc;
  bg->plate_fh = bg->plate_fw = 0;
  HIP_TRY(h, hipMemsetAsync(bg->d_plate, 0, need, s));
  const long cw = bg->canvas_w, ch = bg->canvas_h;
  for (const auto& L : bg->layers) {
    const vss_layer& l = L.l;
    if (l.privacy > bg->level) continue;
    LayerGeom g{};
    g.type = l.type;
    g.X0 = layers_map(l.x, cw, fw);
    g.X1 = layers_map((long)l.x + l.width, cw, fw);
    g.Y0 = layers_map(l.y, ch, fh);
    g.Y1 = layers_map((long)l.y + l.height, ch, fh);
    if (g.X1 <= g.X0 || g.Y1 <= g.Y0) continue;
    if (l.type == VSS_LAYER_ROUNDED_RECT) {
      g.R = std::min(layers_map(l.radius, cw, fw), std::min((g.X1 - g.X0) / 2, (g.Y1 - g.Y0) / 2));
      g.color = (uint32_t)l.color[0] | ((uint32_t)l.color[1] << 8) | ((uint32_t)l.color[2] << 16) |
                ((uint32_t)l.color[3] << 24);
    } else {
      g.sprite = bg->d_sprites + L.sprite_off;
      g.sh = l.src_h; g.sw = l.src_w;
      g.sy = (float)l.src_h / (float)(g.Y1 - g.Y0);
      g.sx = (float)l.src_w / (float)(g.X1 - g.X0);
    }
    if (l.has_shadow) {
      ShadowParams sp{};
      sp.g = g;
      sp.dx = layers_map(l.shadow_dx, cw, fw);
      sp.dy = layers_map(l.shadow_dy, ch, fh);
      const double sigma = (double)l.shadow_blur * (double)fw / (2.0 * (double)cw);
      int r = 3.0 * sigma >= (double)kBlurMaxRadius ? kBlurMaxRadius : (int)std::ceil(3.0 * sigma);
      uint16_t w[2 * kBlurMaxRadius + 1];
      std::string why;
      if (r < 1 || blur_weights(r, sigma, w, &why)) r = 0;  // B = P
      for (int k = 0; k <= r; ++k) sp.w[k] = w[r + k];
      sp.radius = r;
      sp.x0 = clip(g.X0 + sp.dx - r, fw); sp.x1 = clip(g.X1 + sp.dx + r, fw);
      sp.y0 = clip(g.Y0 + sp.dy - r, fh); sp.y1 = clip(g.Y1 + sp.dy + r, fh);
      sp.P = bg->d_shadow;
      sp.Hb = bg->d_shadow + (size_t)pitch * fh;
      sp.pitch = pitch;
      sp.color = (uint32_t)l.shadow_color[0] | ((uint32_t)l.shadow_color[1] << 8) |
                 ((uint32_t)l.shadow_color[2] << 16) | ((uint32_t)l.shadow_color[3] << 24);
      sp.plate = bg->d_plate;
      launch_layer_shadow(sp, s);
    }
    LayerDrawParams d{};
    d.g = g;
    d.x0 = clip(g.X0, fw); d.x1 = clip(g.X1, fw);
    d.y0 = clip(g.Y0, fh); d.y1 = clip(g.Y1, fh);
    d.plate = bg->d_plate;
    d.pitch = pitch;
    launch_layer_draw(d, s);
  }
  if ((rc = launched(h, "layer"))) return rc;
  bg->plate_fh = fh;
  bg->plate_fw = fw;
  return VSS_OK;
}

// bg->mu held; image mode, or colour mode under visible layers (`layered`: O is
// built).  The cached plate d_img for a frame fh x fw: the scaled image, or with
// layers bg' = O over the image or the colour; rebuilt on s when it is stale.
int image_enqueue(vss_handle* h, vss_background* bg, bool layered, int fh, int fw, hipStream_t s) {
  const int mode = bg->mode;
  if (bg->img_fh == fh && bg->img_fw == fw && bg->img_mode == mode && bg->img_layered == layered &&
      !(mode == VSS_BG_COLOR && bg->img_color != bg->color))
    return VSS_OK;
  if (int rc = bg_grow(bg, &bg->d_img, &bg->img_bytes, (size_t)bg_image_stride(fw) * fh)) return rc;
  bg->img_fh = bg->img_fw = 0;
  if (mode == VSS_BG_IMAGE) {
    BgResizeParams r{};
    r.src = bg->d_src;
    r.sh = bg->sh; r.sw = bg->sw; r.sc = bg->sc;
    r.sy = (float)bg->sh / (float)fh;
    r.sx = (float)bg->sw / (float)fw;
    r.out = bg->d_img;
    r.fh = fh; r.fw = fw;
    launch_bg_resize(r, s);
    bg->img_for_image = true;
  }
  if (layered) {
    BgBakeParams b{};
    b.image = bg->d_img;
    b.overlay = bg->d_plate;
    b.fh = fh; b.fw = fw;
    b.from_color = mode == VSS_BG_COLOR;
    b.color = bg->color;
    launch_bg_bake(b, s);
  }
  bg->img_fh = fh;
  bg->img_fw = fw;
  bg->img_mode = mode;
  bg->img_layered = layered;
  bg->img_color = bg->color;
  return VSS_OK;
}

// what a composite refuses an object's settings for, frames fh x fw over a mask H x W (bg->mu held)
int settings_check(vss_handle* h, const vss_background* bg, int fh, int fw, int H, int W) {
  if (bg->mode == VSS_BG_IMAGE && !bg->d_src)
    return fail(h, VSS_E_INVALID_ARG, "background is in image mode but no image was set");
  if (bg->mode == VSS_BG_BLUR && !bg->radius)
    return fail(h, VSS_E_INVALID_ARG, "background is in blur mode but no blur was set");
  if (bg->refine_radius && (fh < H || fw < W))
    return fail(h, VSS_E_INVALID_ARG, "refinement needs a frame no smaller than the mask (" + std::to_string(H) +
                                          " x " + std::to_string(W) + "); turn it off for smaller frames");
  if (bg->refine_radius && W > 16384) return fail(h, VSS_E_INVALID_ARG, "refinement: mask wider than 16384");
  return VSS_OK;
}

}  // namespace

int vss_engine::bg_streams_args(vss_handle* h, vss_background* const* bgs, int n) {
  if (!bgs) return fail(h, VSS_E_INVALID_ARG, "null background array");
  for (int t = 0; t < n; ++t)
    if (!bgs[t] || bgs[t]->h != h)
      return fail(h, VSS_E_INVALID_ARG, "handle / background mismatch at frame " + std::to_string(t));
  return VSS_OK;
}

int vss_engine::bg_streams_check(vss_handle* h, vss_background* const* bgs, int n, int fh, int fw) {
  for (int t = 0; t < n; ++t)
    if (int rc = settings_check(h, bgs[t], fh, fw, h->cfg.model_h, h->cfg.model_w)) return rc;
  return VSS_OK;
}

// Every object's scratch holds one slot per frame of the call that names it;
// frame t uses the slot of its rank among them.  Stale caches are rebuilt per
// object; after that the launch count depends on neither n nor the number of
// objects: per kBgStreamFrames frames the matte stage over the refined frames,
// k_blur_h and the blur form over the blur frames, the flat form over the rest.
int vss_engine::bg_streams_enqueue(vss_handle* h, const BgStreamsLock& lk, vss_background* const* bgs, int n,
                                   const uint8_t* d_frames, int fh, int fw, int fc, size_t rs, size_t fs,
                                   const uint8_t* d_alpha, uint8_t* d_out, size_t ors, size_t ofs, hipStream_t s) {
  const int H = h->cfg.model_h, W = h->cfg.model_w;
  const size_t P = (size_t)H * W, fpx = (size_t)fh * fw;
  // per distinct object: the frames of the call that use it
  std::vector<int> uses(lk.objs.size(), 0), rank((size_t)n), obj((size_t)n);
  for (int t = 0; t < n; ++t) {
    obj[t] = (int)(std::lower_bound(lk.objs.begin(), lk.objs.end(), bgs[t], std::less<vss_background*>()) -
                   lk.objs.begin());
    rank[t] = uses[obj[t]]++;
  }
  std::vector<char> layered(lk.objs.size());
  for (size_t i = 0; i < lk.objs.size(); ++i) {
    vss_background* bg = lk.objs[i];
    // the object's previous composite (and the caches it may have built) may have run on another stream
    int rc = bg->fence.wait_on(h, s);
    if (!rc && bg->refine_radius) rc = bg_grow(bg, &bg->d_matte, &bg->matte_bytes, (size_t)uses[i] * P * 17);
    layered[i] = layers_visible(bg);
    if (!rc && layered[i]) rc = plate_enqueue(h, bg, fh, fw, s);
    if (!rc && (bg->mode == VSS_BG_IMAGE || (bg->mode == VSS_BG_COLOR && layered[i])))
      rc = image_enqueue(h, bg, layered[i], fh, fw, s);
    if (!rc && bg->mode == VSS_BG_BLUR) rc = bg_grow(bg, &bg->d_hblur, &bg->hblur_bytes, (size_t)uses[i] * fpx * 4);
    if (rc) return rc;
  }
  int rc = VSS_OK;
  for (int t0 = 0; t0 < n && !rc; t0 += kBgStreamFrames) {
    const int m = std::min(kBgStreamFrames, n - t0);
    BgStreamsParams p{};
    MatteStreamsParams mp{};
    composite_params(&p.c, d_frames + (size_t)t0 * fs, fh, fw, fc, rs, fs, d_alpha + (size_t)t0 * P, H, W,
                     d_out + (size_t)t0 * ofs, ors, ofs);
    int nflat = 0, nblur = 0, nmatte = 0, max_radius = 0;
    for (int t = 0; t < m; ++t) {
      const vss_background* bg = bgs[t0 + t];
      const size_t k = (size_t)rank[t0 + t], of = (size_t)uses[obj[t0 + t]];  // slot k of `of`
      BgStreamEntry& e = p.entry[t];
      e.color = bg->color;
      if (bg->refine_radius) {
        // the object's planes as for a batch of `of` frames: (abar, bbar), (a_q, b_q), L
        MatteStreamEntry& me = mp.entry[t];
        me.ab = reinterpret_cast<float2*>(bg->d_matte) + k * P;
        me.q = reinterpret_cast<int2*>(bg->d_matte + of * P * 8) + k * P;
        me.L = bg->d_matte + of * P * 16 + k * P;
        me.eps = bg->refine_eps;
        me.radius = bg->refine_radius;
        e.ab = me.ab;
        stream_list_set(mp.list, nmatte++, t);
      }
      if (bg->mode == VSS_BG_BLUR) {
        e.hblur = bg->d_hblur + k * fpx;
        e.overlay = layered[obj[t0 + t]] ? bg->d_plate : nullptr;
        e.taps = bg->d_taps;
        e.radius = bg->radius;
        max_radius = std::max(max_radius, bg->radius);
        stream_list_set(p.blur, nblur++, t);
      } else {
        if (bg->mode == VSS_BG_IMAGE || layered[obj[t0 + t]]) e.image = bg->d_img;  // a colour under layers is a plate too
        stream_list_set(p.flat, nflat++, t);
      }
    }
    if (nmatte) {
      MatteParams& g = mp.m;
      g.frames = p.c.frames;
      g.row_stride = (long)rs;
      g.frame_stride = (long)fs;
      g.fh = fh; g.fw = fw; g.fc = fc;
      g.alpha = p.c.alpha;
      g.H = H; g.W = W;
      launch_matte_streams(mp, nmatte, s);
    }
    launch_bg_streams(p, nflat, nblur, max_radius, s);
    rc = launched(h, "background streams");
  }
  // One event for the call: the first object records it, the others follow it (Fence, vss_engine.h).  Also after
  // a failed launch: what did go out reads the objects' taps, caches and scratch, which a setter may rewrite
  // only after waiting for this event.
  vss_background* first = lk.objs.front();
  const int rr = first->fence.record(h, s);
  if (rr) return rr;
  for (vss_background* bg : lk.objs)
    if (bg != first) bg->fence.follow(first->fence);
  return rc;
}

// bg->mu held.  The fence is recorded only after a composite that went out whole.
int vss_engine::bg_enqueue(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int fh, int fw, int fc,
                           size_t rs, size_t fs, const uint8_t* d_alpha, uint8_t* d_out, size_t ors, size_t ofs,
                           hipStream_t s) {
  if (bg->mode == VSS_BG_IMAGE && !bg->d_src)
    return fail(h, VSS_E_INVALID_ARG, "background is in image mode but no image was set");
  if (bg->mode == VSS_BG_BLUR && !bg->radius)
    return fail(h, VSS_E_INVALID_ARG, "background is in blur mode but no blur was set");
  // the previous composite (and the image it may have scaled) may have run on another stream
  if (int rc = bg->fence.wait_on(h, s)) return rc;
  BgCompositeParams p{};
  composite_params(&p.c, d_frames, fh, fw, fc, rs, fs, d_alpha, h->cfg.model_h, h->cfg.model_w, d_out, ors, ofs);
  p.color = bg->color;
  if (bg->refine_radius) {
    const int rc = matte_enqueue(h, bg, d_frames, n, fh, fw, fc, rs, fs, d_alpha, p.c.H, p.c.W, s, &p.ab);
    if (rc) return rc;
  }
  // branding layers: the overlay plate O, rebuilt here (outside anything captured or replayed) when it is stale
  const bool layered = layers_visible(bg);
  if (layered) {
    const int rc = plate_enqueue(h, bg, fh, fw, s);
    if (rc) return rc;
  }
  int mode = bg->mode;
  if (mode == VSS_BG_IMAGE || (mode == VSS_BG_COLOR && layered)) {
    if (int rc = image_enqueue(h, bg, layered, fh, fw, s)) return rc;
    p.image = bg->d_img;
    mode = VSS_BG_IMAGE;  // a colour under layers is a plate too
  } else if (bg->mode == VSS_BG_BLUR) {
    if (layered) p.overlay = bg->d_plate;
    if (int rc = bg_grow(bg, &bg->d_hblur, &bg->hblur_bytes, (size_t)n * fh * fw * 4)) return rc;
    BlurHParams b{};
    b.frames = d_frames;
    b.row_stride = (long)rs;
    b.frame_stride = (long)fs;
    b.fh = fh; b.fw = fw; b.fc = fc;
    b.out = bg->d_hblur;
    b.radius = bg->radius;
    std::copy(bg->w, bg->w + kBlurMaxRadius + 1, b.w);
    launch_blur_h(b, n, s);
    p.hblur = bg->d_hblur;
    p.radius = bg->radius;
    std::copy(bg->w, bg->w + kBlurMaxRadius + 1, p.w);
  }
  launch_bg_composite(p, mode, n, s);
  if (int rc = launched(h, "background")) return rc;
  return bg->fence.record(h, s);
}

static_assert(VSS_BG_COLOR == kBgColor && VSS_BG_IMAGE == kBgImage && VSS_BG_BLUR == kBgBlur, "modes mirror vss.h");
static_assert(VSS_LAYER_IMAGE == kLayerImage && VSS_LAYER_ROUNDED_RECT == kLayerRect, "layer types mirror vss_layers.h");

extern "C" {

int vss_blur_weights(int radius, double sigma, uint16_t* w) {
  if (!w) return fail(nullptr, VSS_E_INVALID_ARG, "null weights");
  std::string why;
  const int rc = blur_weights(radius, sigma, w, &why);
  return rc ? fail(nullptr, rc, why) : VSS_OK;
}

int vss_background_create(vss_handle* h, vss_background** out) {
  if (!h || !out) return fail(h, VSS_E_INVALID_ARG, "null handle/out");
  *out = nullptr;
  HIP_TRY(h, hipSetDevice(h->device));
  vss_background* bg = new vss_background();
  bg->h = h;
  const hipError_t e = bg->fence.create();
  if (e != hipSuccess) {
    delete bg;
    return fail(h, VSS_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
  }
  *out = bg;
  return VSS_OK;
}

void vss_background_destroy(vss_background* bg) {
  if (!bg) return;
  (void)bg->fence.quiesce(bg->h);
  (void)counted_alloc(bg->h, &bg->d_src, &bg->src_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_img, &bg->img_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_hblur, &bg->hblur_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_taps, &bg->taps_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_matte, &bg->matte_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_sprites, &bg->sprites_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_plate, &bg->plate_bytes, 0);
  (void)counted_alloc(bg->h, &bg->d_shadow, &bg->shadow_bytes, 0);
  bg->fence.destroy();
  delete bg;
}

int vss_background_set_color(vss_background* bg, int r, int g, int b) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  if (r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255)
    return fail(bg->h, VSS_E_INVALID_ARG, "colour components must be in [0, 255]");
  std::lock_guard<std::mutex> lk(bg->mu);
  bg->color = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
  bg->mode = VSS_BG_COLOR;
  return VSS_OK;
}

int vss_background_set_image(vss_background* bg, const uint8_t* pixels, int height, int width, int channels,
                             size_t row_stride) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  vss_handle* h = bg->h;
  if (!pixels) return fail(h, VSS_E_INVALID_ARG, "null image");
  if (height < 1 || width < 1) return fail(h, VSS_E_INVALID_ARG, "bad image size");
  if (channels != 3 && channels != 4) return fail(h, VSS_E_INVALID_ARG, "image channels must be 3 or 4");
  if (row_stride < (size_t)width * channels) return fail(h, VSS_E_INVALID_ARG, "row_stride < width*channels");
  std::lock_guard<std::mutex> lk(bg->mu);
  int rc = bg->fence.quiesce(bg->h);  // a composite may still read the old image
  if (rc) return rc;
  const size_t rb = (size_t)width * channels;
  if ((rc = counted_alloc(bg->h, &bg->d_src, &bg->src_bytes, rb * height))) {
    bg->sh = bg->sw = bg->sc = 0;
    return rc;
  }
  bg->img_fh = bg->img_fw = 0;  // the scaled copy is rebuilt by the next composite
  const hipError_t e = hipMemcpy2D(bg->d_src, rb, pixels, row_stride, rb, height, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)counted_alloc(bg->h, &bg->d_src, &bg->src_bytes, 0);
    return fail(h, VSS_E_HIP, std::string("image upload: ") + hipGetErrorString(e));
  }
  bg->sh = height; bg->sw = width; bg->sc = channels;
  bg->mode = VSS_BG_IMAGE;
  return VSS_OK;
}

int vss_background_set_mode(vss_background* bg, int mode) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  if (mode != VSS_BG_COLOR && mode != VSS_BG_IMAGE && mode != VSS_BG_BLUR)
    return fail(bg->h, VSS_E_INVALID_ARG, "mode must be VSS_BG_COLOR, VSS_BG_IMAGE or VSS_BG_BLUR");
  std::lock_guard<std::mutex> lk(bg->mu);
  bg->mode = mode;
  return VSS_OK;
}

int vss_background_set_blur(vss_background* bg, int radius, double sigma) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  uint16_t w[2 * kBlurMaxRadius + 1];
  std::string why;
  const int rc = blur_weights(radius, sigma, w, &why);
  if (rc) return fail(bg->h, rc, why);
  std::lock_guard<std::mutex> lk(bg->mu);
  // The device copy of the taps, which the calls over many streams read: the object's latest composite may
  // still read the old ones, so this setter waits for it on the host (the others that rewrite device data,
  // set_image and set_layers, always did).
  int rc2 = bg->fence.quiesce(bg->h);
  if (!rc2 && !bg->d_taps) rc2 = counted_alloc(bg->h, &bg->d_taps, &bg->taps_bytes, sizeof(bg->w));
  if (rc2) return rc2;
  uint16_t half[kBlurMaxRadius + 1] = {};
  for (int k = 0; k <= radius; ++k) half[k] = w[radius + k];
  const hipError_t e = hipMemcpy(bg->d_taps, half, sizeof(half), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(bg->h, VSS_E_HIP, std::string("taps upload: ") + hipGetErrorString(e));
  for (int k = 0; k <= radius; ++k) bg->w[k] = half[k];
  bg->radius = radius;
  bg->mode = VSS_BG_BLUR;
  return VSS_OK;
}

int vss_background_set_refine(vss_background* bg, int radius, double eps) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  if (radius < 0 || radius > VSS_REFINE_MAX_RADIUS)
    return fail(bg->h, VSS_E_INVALID_ARG, "refine radius must be 0 (off) or in [1, 8]");
  if (radius && !(eps >= 1.0 && eps <= 65025.0))  // NaN fails both
    return fail(bg->h, VSS_E_INVALID_ARG, "refine eps must be in [1, 65025]");
  std::lock_guard<std::mutex> lk(bg->mu);
  bg->refine_radius = radius;
  bg->refine_eps = radius ? eps : 0.0;
  return VSS_OK;
}

// ---- branding layers (include/vss_layers.h) ----
int vss_layers_map(int v, int canvas, int frame) {
  if (canvas < 1) return 0;
  const long q = layers_map(v, canvas, frame);
  return (int)std::min<long>(std::max<long>(q, INT_MIN), INT_MAX);
}

int vss_background_set_layers(vss_background* bg, const vss_layer* layers, int n, int canvas_w, int canvas_h) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  vss_handle* h = bg->h;
  if (n < 0 || n > VSS_MAX_LAYERS) return fail(h, VSS_E_INVALID_ARG, "layer count must be in [0, 32]");
  if (canvas_w < 1 || canvas_h < 1) return fail(h, VSS_E_INVALID_ARG, "canvas size must be >= 1 x 1");
  if (n > 0 && !layers) return fail(h, VSS_E_INVALID_ARG, "null layer array");
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    const vss_layer& l = layers[i];
    const std::string at = "layer " + std::to_string(i) + ": ";
    if (l.type != VSS_LAYER_IMAGE && l.type != VSS_LAYER_ROUNDED_RECT)
      return fail(h, VSS_E_INVALID_ARG, at + "unknown type");
    if (l.privacy < 1 || l.privacy > 3) return fail(h, VSS_E_INVALID_ARG, at + "privacy must be in [1, 3]");
    if (l.width < 0 || l.height < 0) return fail(h, VSS_E_INVALID_ARG, at + "width and height must be >= 0");
    if (l.radius < 0) return fail(h, VSS_E_INVALID_ARG, at + "radius must be >= 0");
    if (l.shadow_blur < 0) return fail(h, VSS_E_INVALID_ARG, at + "shadow_blur must be >= 0");
    if (l.type == VSS_LAYER_IMAGE) {
      if (!l.pixels) return fail(h, VSS_E_INVALID_ARG, at + "null sprite");
      if (l.src_h < 1 || l.src_h > VSS_LAYER_MAX_SPRITE || l.src_w < 1 || l.src_w > VSS_LAYER_MAX_SPRITE)
        return fail(h, VSS_E_INVALID_ARG, at + "sprite sides must be in [1, 4096]");
      if (l.row_stride < (size_t)l.src_w * 4) return fail(h, VSS_E_INVALID_ARG, at + "row_stride < 4 * src_w");
      total += (size_t)l.src_h * l.src_w * 4;
    }
  }
  // the sprites, premultiplied once: c' = (c*a + 127) / 255
  std::vector<uint8_t> host(total);
  std::vector<vss_background::Layer> fresh((size_t)n);
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    fresh[i].l = layers[i];
    fresh[i].l.pixels = nullptr;
    fresh[i].sprite_off = off;
    if (layers[i].type != VSS_LAYER_IMAGE) continue;
    const vss_layer& l = layers[i];
    for (int y = 0; y < l.src_h; ++y) {
      const uint8_t* src = l.pixels + (size_t)y * l.row_stride;
      uint8_t* dst = host.data() + off + (size_t)y * l.src_w * 4;
      for (int x = 0; x < l.src_w; ++x) {
        const unsigned a = src[4 * x + 3];
        for (int c = 0; c < 3; ++c) dst[4 * x + c] = (uint8_t)((src[4 * x + c] * a + 127u) / 255u);
        dst[4 * x + 3] = (uint8_t)a;
      }
    }
    off += (size_t)l.src_h * l.src_w * 4;
  }
  std::lock_guard<std::mutex> lk(bg->mu);
  int rc = bg->fence.quiesce(bg->h);  // a composite may still read the old sprites and plates
  if (rc) return rc;
  bg->layers.clear();
  bg->plate_fh = bg->plate_fw = 0;  // O and what is baked from it: rebuilt by the next composite
  bg->img_fh = bg->img_fw = 0;
  rc = counted_alloc(bg->h, &bg->d_sprites, &bg->sprites_bytes, total);
  if (!rc && total) {
    const hipError_t e = hipMemcpy(bg->d_sprites, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)counted_alloc(bg->h, &bg->d_sprites, &bg->sprites_bytes, 0);
      rc = fail(h, VSS_E_HIP, std::string("sprite upload: ") + hipGetErrorString(e));
    }
  }
  if (rc) n = 0;  // out of memory or a failed upload: no layers, as after n = 0
  if (n == 0) {
    (void)counted_alloc(bg->h, &bg->d_plate, &bg->plate_bytes, 0);
    (void)counted_alloc(bg->h, &bg->d_shadow, &bg->shadow_bytes, 0);
    // a plate that only a colour under layers needed
    if (!bg->img_for_image) (void)counted_alloc(bg->h, &bg->d_img, &bg->img_bytes, 0);
    bg->img_mode = -1;
    return rc;
  }
  bg->layers = std::move(fresh);
  bg->canvas_w = canvas_w;
  bg->canvas_h = canvas_h;
  return VSS_OK;
}

int vss_background_set_privacy(vss_background* bg, int level) {
  if (!bg) return fail(nullptr, VSS_E_INVALID_ARG, "null background");
  if (level < 1 || level > 3) return fail(bg->h, VSS_E_INVALID_ARG, "privacy level must be in [1, 3]");
  std::lock_guard<std::mutex> lk(bg->mu);
  if (level == bg->level) return VSS_OK;
  bg->level = level;
  bg->plate_fh = bg->plate_fw = 0;
  bg->img_fh = bg->img_fw = 0;
  return VSS_OK;
}

int vss_background_overlay_device(vss_handle* h, vss_background* bg, int height, int width, uint8_t* d_out,
                                  size_t row_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  if (!bg || bg->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / background mismatch");
  if (!d_out) return fail(h, VSS_E_INVALID_ARG, "null device pointer");
  if (height < 1 || width < 1 || height > 16384 || width > 16384)
    return fail(h, VSS_E_INVALID_ARG, "overlay size must be in [1, 16384]");
  if (row_stride < (size_t)width * 4) return fail(h, VSS_E_INVALID_ARG, "row_stride < 4 * width");
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = stream_or(h, stream);
  std::lock_guard<std::mutex> lk(bg->mu);
  int rc = bg->fence.wait_on(h, s);
  if (rc) return rc;
  if (layers_visible(bg)) {
    if ((rc = plate_enqueue(h, bg, height, width, s))) return rc;
    HIP_TRY(h, hipMemcpy2DAsync(d_out, row_stride, bg->d_plate, (size_t)layer_pitch(width) * 4, (size_t)width * 4,
                                height, hipMemcpyDeviceToDevice, s));
  } else {
    HIP_TRY(h, hipMemset2DAsync(d_out, row_stride, 0, (size_t)width * 4, height, s));
  }
  return bg->fence.record(h, s);
}

int vss_background_alpha_device(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int height,
                                int width, int channels, size_t row_stride, size_t frame_stride,
                                const uint8_t* d_alpha_u8, uint8_t* d_out_alpha, size_t out_row_stride,
                                size_t out_frame_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  return vss_background_alpha_device_at(h, bg, d_frames, n, height, width, channels, row_stride, frame_stride,
                                        d_alpha_u8, h->cfg.model_h, h->cfg.model_w, d_out_alpha, out_row_stride,
                                        out_frame_stride, stream);
}

int vss_background_alpha_device_at(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int height,
                                   int width, int channels, size_t row_stride, size_t frame_stride,
                                   const uint8_t* d_alpha_u8, int mask_h, int mask_w, uint8_t* d_out_alpha,
                                   size_t out_row_stride, size_t out_frame_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  if (mask_h < 1 || mask_w < 1) return fail(h, VSS_E_INVALID_ARG, "mask_h / mask_w must be >= 1");
  if (!bg || bg->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / background mismatch");
  if (!d_frames || !d_alpha_u8 || !d_out_alpha) return fail(h, VSS_E_INVALID_ARG, "null device pointer");
  int rc = check_frames(h, n, height, width, channels, row_stride, frame_stride, max_frames(h));
  if (rc) return rc;
  if (out_row_stride < (size_t)width || out_frame_stride < out_row_stride * height)
    return fail(h, VSS_E_INVALID_ARG, "bad alpha output geometry (row stride >= width)");
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = stream_or(h, stream);
  std::lock_guard<std::mutex> lk(bg->mu);
  if ((rc = bg->fence.wait_on(h, s))) return rc;
  MatteAlphaParams p{};
  composite_params(&p.c, d_frames, height, width, channels, row_stride, frame_stride, d_alpha_u8, mask_h, mask_w,
                   d_out_alpha, out_row_stride, out_frame_stride);
  if (bg->refine_radius && (rc = matte_enqueue(h, bg, d_frames, n, height, width, channels, row_stride, frame_stride,
                                               d_alpha_u8, mask_h, mask_w, s, &p.ab)))
    return rc;
  launch_matte_alpha(p, n, s);
  if ((rc = launched(h, "alpha"))) return rc;
  return bg->fence.record(h, s);
}

int vss_background_composite_device(vss_handle* h, vss_background* bg, const uint8_t* d_frames, int n, int height,
                                    int width, int channels, size_t row_stride, size_t frame_stride,
                                    const uint8_t* d_alpha_u8, uint8_t* d_out_rgba, size_t out_row_stride,
                                    size_t out_frame_stride, void* stream) {
  if (!h) return fail(nullptr, VSS_E_INVALID_ARG, "null handle");
  if (!bg || bg->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / background mismatch");
  if (!d_frames || !d_alpha_u8 || !d_out_rgba) return fail(h, VSS_E_INVALID_ARG, "null device pointer");
  int rc = check_frames(h, n, height, width, channels, row_stride, frame_stride, max_frames(h));
  if (rc) return rc;
  if (!rgba_geometry_ok(d_out_rgba, out_row_stride, out_frame_stride, height, width, false))
    return fail(h, VSS_E_INVALID_ARG, "bad RGBA output geometry (row stride >= 4*width, multiple of 4)");
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = stream_or(h, stream);
  std::lock_guard<std::mutex> lk(bg->mu);
  return bg_enqueue(h, bg, d_frames, n, height, width, channels, row_stride, frame_stride, d_alpha_u8, d_out_rgba,
                    out_row_stride, out_frame_stride, s);
}

int vss_segment_background(vss_handle* h, vss_post_state* st, vss_background* bg, const uint8_t* frames, int n,
                           int height, int width, int channels, size_t row_stride, uint8_t* out_rgba) {
  if (!h || !st || st->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / post state mismatch");
  if (!bg || bg->h != h) return fail(h, VSS_E_INVALID_ARG, "handle / background mismatch");
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
  if (!rc) {
    std::lock_guard<std::mutex> bl(bg->mu);
    rc = bg_enqueue(h, bg, s.d_frames, n, height, width, channels, row_stride, fs, h->d_post_u8, h->d_comp, ors, ofs,
                    h->stream);
  }
  return finish_seam(h, lk, k, comp_to_host(h, rc, out_rgba, (size_t)n * ofs));
}

}  // extern "C"
