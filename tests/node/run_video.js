// Driver for tests/test_ts_video.py: NV12 in, NV12 out through the TypeScript
// host (Video.process in segment.js) over a colour background.
//   node run_video.js <y.bin> <uv.bin> <n> <height> <width> <out prefix> <dtype>
'use strict';
const fs = require('fs');
const path = require('path');
const seg = require(path.join(__dirname, '..', '..', 'video-stream-segmenetation_amd', 'ts', 'segment.js'));

async function main() {
  const [yPath, uvPath, n, h, w, outPrefix, dtype] = process.argv.slice(2);
  const N = +n, H = +h, W = +w;
  const yRaw = fs.readFileSync(yPath), uvRaw = fs.readFileSync(uvPath);
  const yb = H * W, ub = (H >> 1) * W;
  const frames = [];
  for (let i = 0; i < N; i++) {
    frames.push({ y: new Uint8Array(yRaw.buffer, yRaw.byteOffset + i * yb, yb),
                  uv: new Uint8Array(uvRaw.buffer, uvRaw.byteOffset + i * ub, ub), width: W, height: H });
  }
  const s = new seg.Segmenter({ dtype: dtype, maxBatch: N, maxFrameWidth: W, maxFrameHeight: H });
  const post = new seg.PostChain(s, {});
  const bg = new seg.Background(s);
  const video = new seg.Video(s, 'bt709');
  await bg.setColor(10, 200, 90);
  const r = await video.process(frames, post, bg);
  fs.writeFileSync(outPrefix + '_y.u8', Buffer.from(r.y.buffer, r.y.byteOffset, r.y.byteLength));
  fs.writeFileSync(outPrefix + '_uv.u8', Buffer.from(r.uv.buffer, r.uv.byteOffset, r.uv.byteLength));
  let badStandard = false, oddRejected = false;
  try { new seg.Video(s, 'bt2020'); } catch (e) { badStandard = e instanceof RangeError; }
  try {
    await video.process([{ y: new Uint8Array(6 * 7), uv: new Uint8Array(3 * 7), width: 7, height: 6 }], post, bg);
  } catch (e) { oddRejected = e.code === '-1'; }
  console.log(JSON.stringify({ width: r.width, height: r.height, count: r.count, badStandardRejected: badStandard,
                               oddWidthRejected: oddRejected }));
  video.close();
  bg.close();
  post.close();
  s.close();
}
main().catch((e) => { console.error(e); process.exit(1); });
