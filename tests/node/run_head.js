// Driver for tests/test_ts_head.py: a multiclass segmentation model through the
// TypeScript host (segment.js InferenceSession / Tensor); every output is
// written back in its own element type.
//   node run_head.js <model.onnx> <inputs.bin> <out prefix>
// inputs.bin holds every input's float32 data, in the session's input order;
// output k is written to <out prefix>_<k>.bin.
'use strict';
const fs = require('fs');
const path = require('path');
const ort = require(path.join(__dirname, '..', '..', 'video-stream-segmenetation_amd', 'ts', 'segment.js'));

async function main() {
  const [modelPath, inputsPath, outPrefix] = process.argv.slice(2);
  const session = await ort.InferenceSession.create(new Uint8Array(fs.readFileSync(modelPath)), {});
  const raw = fs.readFileSync(inputsPath);
  const all = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  const feeds = {};
  let off = 0;
  session.inputNames.forEach((name, i) => {
    const dims = session.inputShapes[i];
    const n = dims.reduce((a, b) => a * b, 1);
    feeds[name] = new ort.Tensor('float32', all.subarray(off, off + n).slice(), dims);
    off += n;
  });
  const out = await session.run(feeds);
  const arrays = session.outputNames.map((name, k) => {
    const t = out[name];
    fs.writeFileSync(`${outPrefix}_${k}.bin`, Buffer.from(t.data.buffer, t.data.byteOffset, t.data.byteLength));
    return t.data.constructor.name;
  });
  // an index output is no feed
  let indexFeedRejected = false;
  const wrong = {};
  wrong[session.inputNames[0]] = out.labels;
  try { await session.run(wrong); } catch (e) { indexFeedRejected = e instanceof TypeError; }
  const headNodes = session.headNodes;
  await session.release();
  console.log(JSON.stringify({
    outputNames: session.outputNames, outputDims: session.outputNames.map((n) => out[n].dims),
    outputTypes: session.outputNames.map((n) => out[n].type), arrays, onnxTypes: session.outputTypes, headNodes,
    indexFeedRejected,
  }));
}
main().catch((e) => { console.error(e); process.exit(1); });
