// node js/bwtcbatchtest.js : BWTC.compressFiles (many independent inputs in one call) through the drop-in module; prints, as JSON,
// the sha256 of every stream of the batch next to that of BWTC.compressFile on the same input (compared by
// tests/test_gpu_js_bwtc_batch.py, for the committed cases also with the golden file).
'use strict';
var crypto = require('crypto');
var cjs = require('./index.js');
function sha(b) { return crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }
function lcg(n, s) {                                  // LCG(n, seed) of SURVEY.md 8c
  var b = Buffer.alloc(n);
  for (var k = 0; k < n; k++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; b[k] = 32 + ((s >>> 16) % 95); }
  return b;
}
var all = Buffer.alloc(256 * 40); for (var i = 0; i < all.length; i++) all[i] = i & 255;
var names = ['empty', 'a1000', 'bytes40', 'lcg30000', 'lcg700000'];
var inputs = [Buffer.alloc(0), Buffer.alloc(1000, 'a'), new Uint8Array(all), lcg(30000, 3), lcg(700000, 5)];   // the last one: two blocks at level 6
var res = { names: names, batch: {}, single: {}, exact: true };
[9, 6, 3].forEach(function(level) {
  var outs = cjs.BWTC.compressFiles(inputs, level);
  res.batch[level] = outs.map(sha);
  res.single[level] = inputs.map(function(x) { return sha(cjs.BWTC.compressFile(x, null, level)); });
  outs.forEach(function(o) { if (!(o instanceof Uint8Array) || o.buffer.byteLength !== o.length) res.exact = false; });
});
res.none = cjs.BWTC.compressFiles([], 9).length;
res.badlevel = cjs.BWTC.compressFiles(inputs.slice(0, 3), 0).map(sha);            // a level outside 1..9 means 9 (lib/BWTC.js:16-19)
console.log(JSON.stringify(res));
