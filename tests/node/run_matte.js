// Driver for tests/test_ts_matte.py: the edge-aware alpha through the TypeScript
// host (Background.setRefine in segment.js): a colour background with
// refinement on, then off again, each on a fresh stream.
//   node run_matte.js <frames.bin> <n> <height> <width> <channels> <out prefix> <dtype>
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
  await bg.setRefine(2, 16);
  const refined = await post.backgroundFrames(frames, bg);
  write('_refined.u8', refined);
  await post.reset();
  await bg.setRefine(0, 0);
  write('_plain.u8', await post.backgroundFrames(frames, bg));
  let rejected = false;
  try { await bg.setRefine(9, 16); } catch (e) { rejected = e.code === '-1'; }
  console.log(JSON.stringify({ width: refined.width, height: refined.height, count: refined.count, badRefineRejected: rejected }));
  bg.close();
  post.close();
  s.close();
}
main().catch((e) => { console.error(e); process.exit(1); });
