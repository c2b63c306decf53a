// node js/batchtest.js : Bzip2.compressFiles (many independent inputs in one call) through the drop-in module; prints, as JSON,
// the sha256 of every stream of the batch next to that of Bzip2.compressFile on the same input (compared by
// tests/test_gpu_js_batch.py, for the committed cases also with the golden file).
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
var names = ['empty', 'a1000', 'bytes40', 'lcg30000', 'mixed120000'];
var mixed = lcg(120000, 11); for (var q = 50000; q < 53000; q++) mixed[q] = 65;      // a long run inside the second input's neighbour
var inputs = [Buffer.alloc(0), Buffer.alloc(1000, 'a'), new Uint8Array(all), lcg(30000, 3), mixed];
var res = { names: names, batch: {}, single: {}, exact: true };
[9, 1].forEach(function(level) {
  var outs = cjs.Bzip2.compressFiles(inputs, level);
  res.batch[level] = outs.map(sha);
  res.single[level] = inputs.map(function(x) { return sha(cjs.Bzip2.compressFile(x, null, level)); });
  outs.forEach(function(o) { if (!(o instanceof Uint8Array) || o.buffer.byteLength !== o.length) res.exact = false; });
});
res.none = cjs.Bzip2.compressFiles([], 9).length;
try { cjs.Bzip2.compressFiles(inputs, 0); res.badlevel = 'no throw'; } catch (e) { res.badlevel = e.message; }
try { cjs.Bzip2.compressFile(inputs[1], null, 0); res.badlevel_single = 'no throw'; } catch (e) { res.badlevel_single = e.message; }
console.log(JSON.stringify(res));
