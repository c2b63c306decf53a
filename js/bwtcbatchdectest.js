// node js/bwtcbatchdectest.js : BWTC.decompressFiles (many independent BWTC streams in one call) through the drop-in module; prints,
// as JSON, the sha256 of every decoded document next to that of its input and of BWTC.decompressFile on the same stream, and what
// damaged streams give (compared by tests/test_gpu_js_bwtc_batch_decode.py).
'use strict';
var crypto = require('crypto');
var cjs = require('./index.js');
function sha(b) { return crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }
function lcg(n, s) {                                  // LCG(n, seed) of SURVEY.md 8c
  var b = Buffer.alloc(n);
  for (var k = 0; k < n; k++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; b[k] = 32 + ((s >>> 16) % 95); }
  return b;
}
function describe(e) { return e instanceof Error ? { message: e.message, index: e.index } : 'no error'; }
var all = Buffer.alloc(256 * 40); for (var i = 0; i < all.length; i++) all[i] = i & 255;
var names = ['empty', 'a1000', 'bytes40', 'lcg30000', 'lcg700000'];
var inputs = [Buffer.alloc(0), Buffer.alloc(1000, 'a'), new Uint8Array(all), lcg(30000, 3), lcg(700000, 5)];   // the last one: two blocks at level 6
var res = { names: names, inputs: inputs.map(sha), batch: {}, single: {}, exact: true };
[9, 6, 3].forEach(function(level) {
  var streams = cjs.BWTC.compressFiles(inputs, level);
  var outs = cjs.BWTC.decompressFiles(streams);
  res.batch[level] = outs.map(sha);
  res.single[level] = streams.map(function(s) { return sha(cjs.BWTC.decompressFile(s)); });
  outs.forEach(function(o) { if (!(o instanceof Uint8Array) || o.buffer.byteLength !== o.length) res.exact = false; });
});
res.none = cjs.BWTC.decompressFiles([]).length;
var good = cjs.BWTC.compressFiles(inputs.slice(1, 4), 8);
var magic = Buffer.from(good[1]); magic[3] ^= 1;
var bad = [good[0], magic, good[2], Buffer.from(good[2]).slice(0, good[2].length - 9)];
try { cjs.BWTC.decompressFiles(bad); res.thrown = 'no throw'; } catch (e) { res.thrown = describe(e); }
try { cjs.BWTC.decompressFile(magic); res.single_thrown = 'no throw'; } catch (e) { res.single_thrown = describe(e); }
try { cjs.BWTC.decompressFile(bad[3]); res.single_cut = 'no throw'; } catch (e) { res.single_cut = describe(e); }
res.kept = cjs.BWTC.decompressFiles(bad, true).map(function(b) { return b instanceof Error ? describe(b) : sha(b); });
console.log(JSON.stringify(res));
