// Driver for tests/test_ts_background.py: virtual backgrounds through the
// TypeScript host (Background and PostChain.backgroundFrames in segment.js):
// a colour, then the blurred frame, each on a fresh stream.
//   node run_background.js <frames.bin> <n> <height> <width> <channels> <out prefix> <dtype>
'use strict';
const fs = require('fs');
const path = require('path');
const seg = require(path.join(__dirname, '..', '..', 'video-stream-segmenetation_amd', 'ts', 'segment.js'));

async function main() {
  const [framesPath, n, h, w, c, outPrefix, dtype] = process.argv.slice(2);
  const N = +n, H = +h, W = +w, C = +c;
  const raw = fs.readFileSync(framesPath);
  const bytes = H * W * C;
  const frames = [];
  for (let i = 0; i < N; i++) {
    frames.push({ data: new Uint8Array(raw.buffer, raw.byteOffset + i * bytes, bytes), width: W, height: H, channels: C });
  }
  const s = new seg.Segmenter({ dtype: dtype, maxBatch: N, maxFrameWidth: W, maxFrameHeight: H });
  const post = new seg.PostChain(s, {});
  const bg = new seg.Background(s);
  const write = (name, r) => fs.writeFileSync(outPrefix + name, Buffer.from(r.rgba.buffer, r.rgba.byteOffset, r.rgba.byteLength));
  await bg.setColor(10, 200, 90);
  const colour = await post.backgroundFrames(frames, bg);
  write('_colour.u8', colour);
  await post.reset();
  await bg.setBlur(7, 2.5);
  write('_blur.u8', await post.backgroundFrames(frames, bg));
  let rejected = false;
  try { await bg.setBlur(0, 1.0); } catch (e) { rejected = e.code === '-1'; }
  console.log(JSON.stringify({ width: colour.width, height: colour.height, count: colour.count, badBlurRejected: rejected }));
  bg.close();
  post.close();
  s.close();
}
main().catch((e) => { console.error(e); process.exit(1); });
