// node js/bwtcbatchdefsumtest.js : BWTC.compressFiles at levels 1 and 5 (DefSumModel on the GPU, k13_defsum_model.hip) through the
// drop-in module; prints, as JSON, the sha256 of every stream of the batch next to that of BWTC.compressFile on the same input
// (compared by tests/test_gpu_js_bwtc_batch_defsum.py).
'use strict';
var crypto = require('crypto');
var cjs = require('./index.js');
function sha(b) { return crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }
function lcg(n, s, lo, span) {                        // LCG(n, seed) of SURVEY.md 8c, over `span` byte values from `lo`
  var b = Buffer.alloc(n);
  for (var k = 0; k < n; k++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; b[k] = lo + ((s >>> 16) % span); }
  return b;
}
var all = Buffer.alloc(256 * 40); for (var i = 0; i < all.length; i++) all[i] = i & 255;
var names = ['empty', 'a1000', 'bytes40', 'lcg30000', 'two20000', 'flat150000'];
var inputs = [Buffer.alloc(0), Buffer.alloc(1000, 'a'), new Uint8Array(all), lcg(30000, 3, 32, 95), lcg(20000, 7, 0, 2),
              lcg(150000, 5, 0, 256)];                // the last one: two blocks at level 1
var res = { names: names, batch: {}, single: {}, exact: true };
[1, 5].forEach(function(level) {
  var outs = cjs.BWTC.compressFiles(inputs, level);
  res.batch[level] = outs.map(sha);
  res.single[level] = inputs.map(function(x) { return sha(cjs.BWTC.compressFile(x, null, level)); });
  outs.forEach(function(o) { if (!(o instanceof Uint8Array) || o.buffer.byteLength !== o.length) res.exact = false; });
});
console.log(JSON.stringify(res));
