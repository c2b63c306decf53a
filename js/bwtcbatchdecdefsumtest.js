// node js/bwtcbatchdecdefsumtest.js : BWTC.decompressFiles on streams of levels 1, 3 and 5 (DefSumModel's decoder on the GPU,
// k14_defsum_decoder.hip) through the drop-in module; prints, as JSON, the sha256 of every decoded document next to that of its
// input, and for a batch with two damaged streams the error objects next to those of BWTC.decompressFile on the same streams
// (compared by tests/test_gpu_js_bwtc_batch_decode_defsum.py).
'use strict';
var crypto = require('crypto');
var cjs = require('./index.js');
function sha(b) { return crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }
function lcg(n, s, lo, span) {                        // LCG(n, seed) of SURVEY.md 8c, over `span` byte values from `lo`
  var b = Buffer.alloc(n);
  for (var k = 0; k < n; k++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; b[k] = lo + ((s >>> 16) % span); }
  return b;
}
function err(f) { try { f(); return null; } catch (e) { return { name: e.name, message: e.message }; } }
var names = ['empty', 'a1000', 'lcg30000', 'two20000', 'flat150000'];
var inputs = [Buffer.alloc(0), Buffer.alloc(1000, 'a'), lcg(30000, 3, 32, 95), lcg(20000, 7, 0, 2), lcg(150000, 5, 0, 256)];   // the last one: two blocks at level 1
var res = { names: names, input: inputs.map(sha), decoded: {}, exact: true };
var streams = {};
[1, 3, 5].forEach(function(level) {
  streams[level] = cjs.BWTC.compressFiles(inputs, level);
  var outs = cjs.BWTC.decompressFiles(streams[level]);
  res.decoded[level] = outs.map(sha);
  outs.forEach(function(o) { if (!(o instanceof Uint8Array)) res.exact = false; });
});
// damaged streams among good ones of three levels: a flipped magic, a truncation
var magic = Buffer.from(streams[3][1]); magic[2] ^= 0x10;
var cut = Buffer.from(streams[5][2]).slice(0, streams[5][2].length - 11);
var bad = [streams[1][1], magic, streams[3][2], cut, streams[5][3]];
var got = cjs.BWTC.decompressFiles(bad, true);
res.mixed = got.map(function(g, i) { return g instanceof Error ? { name: g.name, message: g.message, index: g.index } : sha(g); });
res.mixed_single = bad.map(function(s) { var out = null; var e = err(function() { out = cjs.BWTC.decompressFile(s); }); return e ? e : sha(out); });
res.thrown = err(function() { cjs.BWTC.decompressFiles(bad); });
console.log(JSON.stringify(res));
