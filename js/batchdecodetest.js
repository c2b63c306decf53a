// node js/batchdecodetest.js : Bzip2.decompressFiles (many independent .bz2 inputs in one call) through the drop-in module.  Ten
// documents, two of them corrupt (a flipped block-CRC bit, a truncation); prints, as JSON, the sha256 of every Buffer of the batch
// next to that of Bzip2.decompressFile on the same input, and what the batch throws / returns for the corrupt ones next to what
// decompressFile throws (compared by tests/test_gpu_js_batch_decode.py).
'use strict';
var crypto = require('crypto');
var cjs = require('./index.js');
function sha(b) { return crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }
function lcg(n, s) {                                  // LCG(n, seed) of SURVEY.md 8c
  var b = Buffer.alloc(n);
  for (var k = 0; k < n; k++) { s = (Math.imul(s, 1664525) + 1013904223) >>> 0; b[k] = 32 + ((s >>> 16) % 95); }
  return b;
}
function describe(e) { return { ctor: e.constructor.name, errorCode: e.errorCode, message: e.message, index: e.index }; }
var inputs = [Buffer.alloc(0), Buffer.alloc(1000, 'a'), lcg(30000, 3), lcg(7, 4), lcg(250000, 5), lcg(300, 6), lcg(2000, 7), Buffer.alloc(70000, 'z'),
              lcg(99981, 8), lcg(1, 9)];
var streams = cjs.Bzip2.compressFiles(inputs, 1).map(function(u) { return Buffer.from(u); });
var good = streams.slice();
streams[3] = Buffer.from(streams[3]); streams[3][4 + 6 + 1] ^= 0x10;            // a bit of the stored block CRC
streams[6] = streams[6].slice(0, streams[6].length - 11);                        // truncated
var res = { inputs: inputs.map(sha), bad: [3, 6] };
res.batch = cjs.Bzip2.decompressFiles(good).map(function(b) { return Buffer.isBuffer(b) ? sha(b) : 'not a Buffer'; });
res.single = good.map(function(s) { return sha(cjs.Bzip2.decompressFile(s)); });
res.none = cjs.Bzip2.decompressFiles([]).length;
res.single_err = {};
res.bad.forEach(function(k) { try { cjs.Bzip2.decompressFile(streams[k]); res.single_err[k] = 'no throw'; } catch (e) { res.single_err[k] = describe(e); } });
try { cjs.Bzip2.decompressFiles(streams); res.thrown = 'no throw'; } catch (e) { res.thrown = describe(e); }
res.kept = cjs.Bzip2.decompressFiles(streams, false, true).map(function(b) { return Buffer.isBuffer(b) ? sha(b) : describe(b); });
console.log(JSON.stringify(res));
