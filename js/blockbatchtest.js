// node js/blockbatchtest.js <stream.bz2> <positions.json> : Bzip2.decompressBlocks (many blocks of one stream in one call) through the
// drop-in module.  positions.json is an array of decimal strings (bit positions up to 2^64 - 1: BigInt above 2^53).  Prints, as JSON,
// the sha256 of every Buffer - or the error - of the call with returnErrors, what the call without it throws, and for the first few
// positions what Bzip2.decompressBlock gives (compared by tests/test_gpu_js_block_batch.py with the oracle's digests).
'use strict';
var crypto = require('crypto');
var fs = require('fs');
var cjs = require('./index.js');
function sha(b) { return crypto.createHash('sha256').update(Buffer.from(b)).digest('hex'); }
function describe(e) { return { ctor: e.constructor.name, errorCode: e.errorCode, message: e.message, index: e.index }; }
var stream = fs.readFileSync(process.argv[2]);
var pos = JSON.parse(fs.readFileSync(process.argv[3], 'utf8')).map(function(s) {
  var b = BigInt(s);
  return b <= BigInt(Number.MAX_SAFE_INTEGER) ? Number(b) : b;
});
var res = { count: pos.length };
res.kept = cjs.Bzip2.decompressBlocks(stream, pos, true).map(function(b) { return Buffer.isBuffer(b) ? sha(b) : describe(b); });
try { cjs.Bzip2.decompressBlocks(stream, pos); res.thrown = 'no throw'; } catch (e) { res.thrown = describe(e); }
res.none = cjs.Bzip2.decompressBlocks(stream, []).length;
res.single = pos.slice(0, 12).map(function(p) {
  if (typeof p !== 'number') return 'skipped';
  try { return sha(cjs.Bzip2.decompressBlock(stream, p)); } catch (e) { return describe(e); }
});
console.log(JSON.stringify(res));
