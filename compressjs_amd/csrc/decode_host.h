// Host entry points of the GPU bzip2 decoder (decode.hip), used by the C ABI (cjs_abi.hip).
#pragma once
#include "cjs_common.h"

struct DecState;
void dec_free(DecState* S);
// Bunzip.decode: returns the decoded size (bytes stay in the decoder's HBM buffer) or an Err code
int64_t dec_stream(DecState** ps, u32 slots, hipStream_t st, const u8* in, u64 len, bool in_dev, int multistream,
                   bool check_stream_crc);
// Bunzip.decodeBlock on a host buffer
int64_t dec_block(DecState** ps, u32 slots, hipStream_t st, const u8* in, u64 len, u64 bitpos);
// a batch of documents (cjs_bz2_decompress_batch): document d = in[off[d], off[d+1]) decodes as dec_stream does on it alone.  dev:
// in / off / out_off / status / detail are device pointers.  Returns the total of decoded bytes (they stay in the decoder's buffer,
// failed documents contributing none) or a call-level error; per-document outcomes go to out_off / status / detail (may be null).
int64_t dec_batch(DecState** ps, u32 slots, hipStream_t st, const u8* in, const u64* off, u32 count, bool dev, int multistream,
                  u64* out_off, int* status, u32* detail);
// a list of blocks of one stream (cjs_bz2_decompress_blocks): request k decodes as dec_block does at bitpos[k] alone, without its
// call-level errors: a bad stream header fails every request.  dev: in / bitpos / out_off / status / detail are device pointers.
// Returns and delivers as dec_batch does, one record per request.
int64_t dec_blocks(DecState** ps, u32 slots, hipStream_t st, const u8* in, u64 len, const u64* bitpos, u32 count, bool dev,
                   u64* out_off, int* status, u32* detail);
// host<->device synchronisations of the last decode call (dec_sync_note: one more, made by the caller on its behalf)
int dec_sync_count();
void dec_sync_note();
const u8* dec_output(DecState* S, u64* size);
void dec_error_info(DecState* S, int* detail, u32* got, u32* want);
u32 dec_table(DecState* S, const u64** pos, const u64** size);
