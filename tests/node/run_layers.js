// Driver for tests/test_ts_layers.py: branding layers through the TypeScript
// host (Background.setLayers / setPrivacy in segment.js): a blurred frame, then
// an image, each under the same layers on a fresh stream.
//   node run_layers.js <frames.bin> <n> <height> <width> <channels> <sprite.bin> <sh> <sw> <image.bin> <ih> <iw> <out prefix> <dtype>
'use strict';
const fs = require('fs');
const path = require('path');
const seg = require(path.join(__dirname, '..', '..', 'video-stream-segmenetation_amd', 'ts', 'segment.js'));

async function main() {
  const [framesPath, n, h, w, c, spritePath, sh, sw, imagePath, ih, iw, outPrefix, dtype] = process.argv.slice(2);
  const N = +n, H = +h, W = +w, C = +c;
  const raw = fs.readFileSync(framesPath);
  const bytes = H * W * C;
  const frames = [];
  for (let i = 0; i < N; i++) {
    frames.push({ data: new Uint8Array(raw.buffer, raw.byteOffset + i * bytes, bytes), width: W, height: H, channels: C });
  }
  const sprite = new Uint8Array(fs.readFileSync(spritePath));
  const image = new Uint8Array(fs.readFileSync(imagePath));
  const layers = [
    { type: 'rect', privacy: 'low', x: 50, y: 90, width: 1100, height: 280, color: [0, 0, 0, 64], radius: 20 },
    { type: 'image', privacy: 'medium', x: 300, y: 200, width: 900, height: 500, pixels: sprite, srcHeight: +sh, srcWidth: +sw,
      shadow: { color: [0, 0, 0, 179], blur: 40, dx: 20, dy: 20 } },
    { type: 'rect', privacy: 'high', x: 1300, y: 60, width: 580, height: 350, color: [250, 10, 20, 200], radius: 60 },
  ];
  const s = new seg.Segmenter({ dtype: dtype, maxBatch: N, maxFrameWidth: W, maxFrameHeight: H });
  const post = new seg.PostChain(s, {});
  const bg = new seg.Background(s);
  const write = (name, r) => fs.writeFileSync(outPrefix + name, Buffer.from(r.rgba.buffer, r.rgba.byteOffset, r.rgba.byteLength));
  await bg.setBlur(7, 2.5);
  await bg.setLayers(layers);
  const blur = await post.backgroundFrames(frames, bg);
  write('_blur.u8', blur);
  await post.reset();
  await bg.setImage({ data: image, height: +ih, width: +iw, channels: 3 });
  await bg.setPrivacy('high');
  write('_image.u8', await post.backgroundFrames(frames, bg));
  let rejected = 0;
  try { await bg.setPrivacy(4); } catch (e) { rejected += e.code === '-1' ? 1 : 0; }
  try { await bg.setLayers([{ type: 'rect', privacy: 1, x: 0, y: 0, width: -1, height: 5 }]); } catch (e) { rejected += e.code === '-1' ? 1 : 0; }
  console.log(JSON.stringify({ width: blur.width, height: blur.height, count: blur.count, rejected: rejected }));
  bg.close();
  post.close();
  s.close();
}
main().catch((e) => { console.error(e); process.exit(1); });
