// Driver for tests/test_ts_pool.py: the post chain over many streams through the
// TypeScript host (PostPool in segment.js).  Frames 0-2 go to streams 3, 0, 1 in
// one call, frames 3-4 to streams 1, 3 in the next; then stream 3 is reset and
// given frame 0 again.
//   node run_pool.js <frames.bin> <height> <width> <channels> <out prefix> <dtype>
'use strict';
const fs = require('fs');
const path = require('path');
const seg = require(path.join(__dirname, '..', '..', 'video-stream-segmenetation_amd', 'ts', 'segment.js'));

async function main() {
  const [framesPath, h, w, c, outPrefix, dtype] = process.argv.slice(2);
  const H = +h, W = +w, C = +c;
  const raw = fs.readFileSync(framesPath);
  const bytes = H * W * C;
  const frames = [];
  for (let i = 0; i < 5; i++) {
    frames.push({ data: new Uint8Array(raw.buffer, raw.byteOffset + i * bytes, bytes), width: W, height: H, channels: C });
  }
  const s = new seg.Segmenter({ dtype: dtype, maxBatch: 3, maxFrameWidth: W, maxFrameHeight: H });
  const pool = new seg.PostPool(s, 4, {});
  const parts = [];
  parts.push(await pool.segment([3, 0, 1], frames.slice(0, 3)));
  parts.push(await pool.segment([1, 3], frames.slice(3, 5)));
  await pool.reset(3);
  parts.push(await pool.segment([3], frames.slice(0, 1)));
  let dupRejected = false, rangeRejected = false, countRejected = false;
  try { await pool.segment([2, 2], frames.slice(0, 2)); } catch (e) { dupRejected = e.code === '-1'; }
  try { await pool.segment([4], frames.slice(0, 1)); } catch (e) { rangeRejected = e.code === '-1'; }
  try { await pool.segment([1], frames.slice(0, 2)); } catch (e) { countRejected = e instanceof RangeError; }
  await pool.reset();
  await pool.setConfig({ USE_BILATERAL: false, GAMMA: 1.0 });
  parts.push(await pool.segment([0, 2], frames.slice(1, 3)));
  let count = 0;
  for (const p of parts) count += p.count;
  const px = parts[0].width * parts[0].height;
  const alpha = new Float32Array(count * px), u8 = new Uint8Array(count * px);
  let at = 0;
  for (const p of parts) {
    alpha.set(p.alpha, at);
    u8.set(p.alphaU8, at);
    at += p.count * px;
  }
  fs.writeFileSync(outPrefix + '.f32', Buffer.from(alpha.buffer));
  fs.writeFileSync(outPrefix + '.u8', Buffer.from(u8.buffer));
  console.log(JSON.stringify({ width: parts[0].width, height: parts[0].height, count: count,
                               dupRejected: dupRejected, rangeRejected: rangeRejected, countRejected: countRejected }));
  pool.close();
  s.close();
}
main().catch((e) => { console.error(e); process.exit(1); });
