/*
 * turbopfor_gpu.h -- C-ABI of the MI355X (gfx950) P4 codec: batched device
 * entry points.  Plain C types only (no HIP/torch types): `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  All pointers named
 * d_* are device pointers; inputs are expected to be resident in HBM.
 *
 * Layout contract for the batched 256v32 / 256v64 formats:
 *   - the packed stream is the reference's per-block encodings laid end to
 *     end, exactly as the reference's callers chain them with the returned end
 *     pointer (README.md:108-123);
 *   - d_off[0..nblocks] are byte offsets of each block (d_off[nblocks] = end);
 *     the reference has no offsets (block sizes are implicit), so the batch
 *     encoders produce them and tpf_scan_offsets recovers them from a legacy
 *     stream;
 *   - OFFSETS CONTRACT (every entry below that takes d_off / h_off): the
 *     array has nblocks + 1 readable entries.  The kernels read d_off[i] and
 *     d_off[i+1] of every block they decode; the array's length is not passed
 *     and cannot be checked on the device, so a shorter array is an
 *     out-of-bounds device read (round 5 saw one fault from a test that broke
 *     this).  The VALUES are checked: an offset outside [0, in_bytes] or a
 *     block whose parse disagrees with its offsets is reported through d_err,
 *     never followed;
 *   - decoded values are nblocks * 256 contiguous integers.
 * No device-side slack is required: all device reads are bounds-checked
 * against in_bytes, and no byte at or after d_in + in_bytes can change a
 * result (d_in may start at any byte address).
 *
 * WORKSPACE CONTRACT (every codec entry point below that takes d_ws; the lists
 * entry points state the same for themselves):
 *   - d_ws holds at least the bytes the matching *_workspace_size export
 *     returns for the same counts and is at least 8-byte aligned; a smaller
 *     ws_bytes is TPF_EINVAL ("workspace too small") and nothing is enqueued,
 *     not even the initialisation of d_err.  The exports are multiples of 256
 *     and non-decreasing in their count, so one buffer sized for the largest
 *     batch serves every smaller one;
 *   - nothing outside [d_ws, d_ws + size export) is read or written;
 *   - its contents on entry are irrelevant: no call relies on what it, or any
 *     other call, left there;
 *   - the next call on the same stream may reuse it at once, without a
 *     synchronisation in between -- but for a chain_decode, which reads what
 *     the chain_sums before it wrote (below);
 *   - a call may be captured into a hipGraph and replayed on a workspace
 *     that was overwritten in between.
 * OUTPUT CONTRACT: a decoder writes exactly the values its section names
 * (nblocks * 256, nunits * width, nblocks * n for the horizontal formats, n
 * for an n-variant stream) and nothing before or after them; d_off is count +
 * 1 entries, d_err one u64, d_total one element.  Every encoder writes
 * d_off[0..count] and the stream's d_off[count] bytes of d_out: the bytes of
 * d_out between the stream's end and out_cap are left untouched, on every
 * route (tests/test_gpu_codec_workspace.py holds all of this).
 *
 * Return value: TPF_OK (0) or a negative TPF_E* code; tpf_last_error()
 * returns a thread-local message for the last failure.
 */
#ifndef TURBOPFOR_GPU_H
#define TURBOPFOR_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPF_OK 0
#define TPF_EINVAL (-1)  /* bad argument */
#define TPF_EHIP (-2)    /* HIP runtime error (see tpf_last_error) */
#define TPF_ENODEV (-3)  /* no HIP device: the library has no CPU fallback */
#define TPF_ECORRUPT (-4) /* a block's parsed length disagrees with its offsets */

const char *tpf_last_error(void);
int tpf_device_count(void);

/* ---- 256v32 decode (hot path) ------------------------------------------
 * Replaces per-block turbopfor::p4Dec256v32 (reference include/turbopfor.h:39,
 * src/dispatch.cpp:88-95).  d_err (optional, may be NULL): receives the index
 * of the first block whose parsed byte length differs from
 * d_off[i+1]-d_off[i], or UINT64_MAX when every block is consistent. */
int tpf_p4dec256v32_batch(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nblocks,
                          uint32_t *d_out, uint64_t *d_err, void *stream);


/* Replaces turbopfor::p4D1Dec256v32 (include/turbopfor.h:42, dispatch.cpp:97-104):
 * block i is decoded with start d_starts[i] (the value preceding the block). */
int tpf_p4d1dec256v32_batch(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nblocks,
                            uint32_t *d_out, const uint32_t *d_starts, uint64_t *d_err, void *stream);

/* ---- 256v32 chained delta-1 decode -------------------
 * One posting list split into nblocks consecutive 256v32 D1 blocks, encoded
 * the way reference callers chain them (start of block i = last value of
 * block i-1, README.md:116-123): decode the whole list on the device with
 * only the list's initial start0.  Phase A (chain_sums) decodes every block's
 * delta sum and prefix-sums them into the workspace; phase B (chain_decode)
 * decodes with start(i) = base + prefix(i-1).  tpf_p4d1dec256v32_chained = A+B
 * with base = start0.  For a list sharded over GPUs, each rank runs A, the
 * ranks exchange their totals (d_total, one u32 each) and each runs B with
 * base = start0 + the totals of all earlier shards (mod 2^32).
 * d_ws: tpf_p4d1dec256v32_chain_workspace_size(nblocks) bytes under the
 * WORKSPACE CONTRACT above.  chain_decode only reads it: it may run any number
 * of times, with any base, against one chain_sums, and leaves every byte as
 * phase A wrote it. */
size_t tpf_p4d1dec256v32_chain_workspace_size(uint64_t nblocks);
int tpf_p4d1dec256v32_chained(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nblocks,
                              uint32_t *d_out, uint32_t start0, void *d_ws, size_t ws_bytes, uint64_t *d_err,
                              void *stream);
int tpf_p4d1dec256v32_chain_sums(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nblocks,
                                 void *d_ws, size_t ws_bytes, uint32_t *d_total, uint64_t *d_err, void *stream);
int tpf_p4d1dec256v32_chain_decode(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nblocks,
                                   uint32_t *d_out, uint32_t base, const void *d_ws, uint64_t *d_err, void *stream);

/* ---- 64-bit chained delta-1 decode (128v64 / 256v64) --------------------
 * The 64-bit counterpart of the chained 256v32 decode: nunits consecutive
 * p4D1Enc256v64 (fmt TPF_FMT_256V64, 256 values per unit) or p4D1Enc128v64
 * (TPF_FMT_128V64, 128) units chained the way reference callers chain them
 * (start of unit i = last value of unit i-1, README.md:116-123; reference
 * decoder p4d1dec256v64_scalar.cpp:15-32, which carries the start across its
 * two 128-value blocks the same way).  Phase A (chain_sums) decodes every
 * unit's delta total sum(v + 1) mod 2^64 and prefix-sums them into the
 * workspace; phase B (chain_decode) decodes with start(i) = base + the totals
 * before i.  tpf_d1dec64_chained = A + B with base = start0; for a sharded list
 * exchange the d_total of each shard (one u64) as for 256v32.  d_out: nunits *
 * 128 * (1 or 2) u64.  d_ws: tpf_d1dec64_chain_workspace_size(nunits) bytes
 * under the WORKSPACE CONTRACT above; chain_decode only reads it. */
size_t tpf_d1dec64_chain_workspace_size(uint64_t nunits);
int tpf_d1dec64_chained(int fmt, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                        uint64_t *d_out, uint64_t start0, void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);
int tpf_d1dec64_chain_sums(int fmt, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                           void *d_ws, size_t ws_bytes, uint64_t *d_total, uint64_t *d_err, void *stream);
int tpf_d1dec64_chain_decode(int fmt, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                             uint64_t *d_out, uint64_t base, const void *d_ws, uint64_t *d_err, void *stream);
/* Named forms: replace a caller's loop of turbopfor::p4D1Dec256v64 /
 * p4D1Dec128v64 calls (include/turbopfor.h:80,67) over one chained list. */
int tpf_p4d1dec256v64_chained(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                              uint64_t *d_out, uint64_t start0, void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);
int tpf_p4d1dec128v64_chained(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                              uint64_t *d_out, uint64_t start0, void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- 256v32 encode ---------------------------------------------------
 * Replaces turbopfor::p4Enc256v32 (include/turbopfor.h:33, dispatch.cpp:70-77)
 * and p4D1Enc256v32 (:36, dispatch.cpp:79-86) for nblocks blocks of 256
 * values (d_in: nblocks*256 u32).  Writes the blocks end to end into d_out
 * (capacity out_cap bytes, at least tpf_p4enc256v32_bound(nblocks): the
 * sizes are only known on the device, so a smaller out_cap is rejected with
 * TPF_EINVAL instead of risking a silently cut-off block)
 * and their byte offsets into d_off[0..nblocks] (d_off[nblocks] = total).
 * d_ws: device workspace of tpf_p4enc256v32_workspace_size(nblocks) bytes
 * under the WORKSPACE CONTRACT above.  Bytes of d_out past d_off[nblocks] are
 * left untouched.
 * D1: d_starts[i] is the value preceding block i; with d_starts == NULL the
 * blocks are one chained posting list: block 0 starts from start0 and block
 * i>0 from the last input value of block i-1. */
uint64_t tpf_p4enc256v32_bound(uint64_t nblocks);
size_t tpf_p4enc256v32_workspace_size(uint64_t nblocks);
int tpf_p4enc256v32_batch(const uint32_t *d_in, uint64_t nblocks, uint8_t *d_out, uint64_t out_cap, uint64_t *d_off,
                          void *d_ws, size_t ws_bytes, void *stream);
int tpf_p4d1enc256v32_batch(const uint32_t *d_in, uint64_t nblocks, const uint32_t *d_starts, uint32_t start0,
                            uint8_t *d_out, uint64_t out_cap, uint64_t *d_off, void *d_ws, size_t ws_bytes, void *stream);

/* ---- every format of include/turbopfor.h, batched ----------------------
 * fmt selects the reference function family:
 *   TPF_FMT_32     p4{,D1}{Enc,Dec}32      (turbopfor.h:9-18)   n = 1..256 values per block
 *   TPF_FMT_128V32 p4{,D1}{Enc,Dec}128v32  (turbopfor.h:21-30)  n <= 128
 *   TPF_FMT_256V32 p4{,D1}{Enc,Dec}256v32  (turbopfor.h:33-42)  n <= 256 (n == 256 -> hot path)
 *   TPF_FMT_64     p4{,D1}{Enc,Dec}64      (turbopfor.h:45-54)  n = 1..256 (uint64)
 *   TPF_FMT_128V64 p4{,D1}{Enc,Dec}128v64  (turbopfor.h:57-67)  n <= 128 (uint64)
 *   TPF_FMT_256V64 p4{,D1}{Enc,Dec}256v64  (turbopfor.h:69-80)  n == 256 (uint64; one unit = two 128v64 blocks;
 *                  the per-block turbopfor::p4*256v64 calls take any n and split it into 128v64 blocks
 *                  of min(remaining, 128) values like the reference, p4enc256v64_scalar.cpp:15-30)
 * A batch holds nblocks units; unit i's values are at d_vals + i*stride with
 * stride = n for the horizontal formats and the layout's full width (128 or
 * 256) for the interleaved ones (the reference packs the full width).
 * PADDING CONTRACT (TPF_FMT_128V32 / TPF_FMT_256V32 with n below the width):
 * without delta-1 a block the encoder leaves in plain mode (header b, no
 * exceptions) carries the low b bits of the caller's slots n .. width-1, as
 * the reference's p4Enc128v32 / p4Enc256v32 do; no other mode, and no length,
 * depends on those slots.  With delta-1 they are never read: the padding
 * bits are zero (the reference packs its uninitialised stack there,
 * p4d1enc128v32_scalar.cpp:12) and the next unit of a chained list starts
 * from value n-1.  Of a decoded unit the first n values are specified
 * (tests/test_gpu_formats32.py holds all of this).
 * TPF_FMT_128V64 with n below 128 follows the same contract on both of its
 * base layouts: without delta-1 a plain-mode block carries the low b bits of
 * the caller's slots n .. 127 -- in the pair-swapped 128v32 layout at
 * b <= 32, in the horizontal 64-bit pack at b > 32, the whole words at width
 * 64 (header 63) -- as the reference's p4Enc128v64 does, which hands the
 * caller's array to bitpack128v64Scalar and that packs 128 slots
 * (p4enc128v64_scalar.cpp:167); no other mode, and no length, depends on
 * those slots.  With delta-1, and in the base payload of every bitmap or
 * vbyte block, the padding bits are zero (the reference packs its
 * uninitialised stack there, p4enc128v64_scalar.cpp:59,
 * p4d1enc128v64_scalar.cpp) and the next unit of a chained list starts from
 * value n-1 (tests/test_gpu_formats64.py).  TPF_FMT_256V64 batches hold
 * whole units (n = 256).
 * Values are uint32 or uint64 as the family requires.  D1 (delta-1): starts
 * per unit, or NULL = one chained list (encode: start0 then the previous
 * unit's last input, value n-1; decode requires starts). */
#define TPF_FMT_32 0
#define TPF_FMT_128V32 1
#define TPF_FMT_256V32 2
#define TPF_FMT_64 3
#define TPF_FMT_128V64 4
#define TPF_FMT_256V64 5

/* tpf_enc_batch requires out_cap >= tpf_enc_bound(fmt, nblocks, n) (TPF_EINVAL otherwise).
 * tpf_dec_batch reports through d_err (first such block index) any block whose
 * parse disagrees with its offsets; for TPF_FMT_32 (the windowed decoder) also
 * any block whose offsets span more than 2,544 bytes or run past in_bytes --
 * a p4Enc32 block of n <= 256 values is at most about 1 KB.
 * tpf_enc_batch's d_ws: tpf_enc_workspace_size(fmt, nblocks, n) bytes under
 * the WORKSPACE CONTRACT above, on each of its three routes (256v32 with n ==
 * 256; 128v64 with n == 128 and 256v64; every other (fmt, n)); bytes of d_out
 * past d_off[nblocks] are left untouched.  tpf_dec_batch takes no workspace
 * and writes nblocks * stride values (stride as above), nothing after them. */
uint64_t tpf_enc_bound(int fmt, uint64_t nblocks, unsigned n);
size_t tpf_enc_workspace_size(int fmt, uint64_t nblocks, unsigned n);
int tpf_dec_batch(int fmt, const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nblocks, unsigned n,
                  void *d_vals, const void *d_starts, uint64_t *d_err, void *stream);
int tpf_enc_batch(int fmt, const void *d_vals, uint64_t nblocks, unsigned n, int d1, const void *d_starts, uint64_t start0,
                  uint8_t *d_out, uint64_t out_cap, uint64_t *d_off, void *d_ws, size_t ws_bytes, void *stream);

/* ---- n-variant streams --------------------------------
 * n values of any count as floor(n/256) p4Enc256v32 blocks followed, when
 * n % 256 != 0, by one p4Enc32 block of the remaining values: the stream a
 * caller produces by chaining turbopfor::p4Enc256v32 over the full blocks
 * and turbopfor::p4Enc32 over the tail (reference include/turbopfor.h:9,
 * :33; D1: p4D1Enc256v32 / p4D1Enc32 with each block's start = the value
 * before it, the first = start0).  d_off receives nunits + 1 byte offsets
 * (nunits = n/256 + (n%256 != 0)); d_off[nunits] is the stream's length.
 * Decode takes the same offsets (tpf_scan_offsets of the parts, or the
 * encoder's) and writes exactly n values.
 * d_ws: tpf_p4nenc256v32_workspace_size(n) / tpf_p4ndec256v32_workspace_size(n)
 * bytes under the WORKSPACE CONTRACT above (both keep u64 words in its first
 * 256 bytes, hence the 8-byte alignment); the encoder leaves the bytes of
 * d_out past d_off[nunits] untouched. */
uint64_t tpf_p4nenc256v32_bound(uint64_t n);
size_t tpf_p4nenc256v32_workspace_size(uint64_t n);
int tpf_p4nenc256v32(const uint32_t *d_in, uint64_t n, int d1, uint32_t start0, uint8_t *d_out, uint64_t out_cap,
                     uint64_t *d_off, void *d_ws, size_t ws_bytes, void *stream);
size_t tpf_p4ndec256v32_workspace_size(uint64_t n);
int tpf_p4ndec256v32(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t n, int d1, uint32_t start0,
                     uint32_t *d_out, void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- many lists in one call ------------------------------------------------
 * An inverted index is a very large number of posting lists of very different
 * lengths, each stored as the n-variant stream above: a caller's chain of
 * p4{,D1}Enc256v32 over the full 256-value blocks and p4{,D1}Enc32 over the
 * last n % 256 values (reference include/turbopfor.h:9, :33), every block's
 * start the value before it.  tpf_p4ndec256v32_lists decodes nlists such
 * streams laid end to end in ONE submission (replacing a loop of
 * tpf_p4ndec256v32 calls, a handful of launches per list).
 *   - List layout (CSR form): d_list_ptr[0..nlists] is non-decreasing; list j
 *     has n_j = ptr[j+1] - ptr[j] values, written to d_out + ptr[j], so the
 *     output is dense and ragged.  ptr[0] need not be 0.  Empty lists are
 *     allowed anywhere, any number in a row.
 *   - Units: list j occupies units_j = n_j/256 + (n_j%256 != 0) consecutive
 *     units of the stream, in list order: its full 256v32 blocks, then one
 *     p4{,D1}Enc32 block of n_j % 256 values -- the stream tpf_p4nenc256v32
 *     writes for one list, the lists concatenated.
 *   - Offsets: d_off[0..nunits] are the units' byte offsets under the OFFSETS
 *     CONTRACT above (nunits + 1 readable entries); nunits must equal the sum
 *     of units_j.
 *   - Delta-1: with d1 != 0 list j is chained from d_start0[j] (the value
 *     before its first); d_start0 == NULL means 0 for every list.  Arithmetic
 *     is mod 2^32 as in the reference's applyDelta1_256.  With d1 == 0
 *     d_start0 is ignored.
 *   - Output bounds: out_values is the capacity of d_out in values; nothing is
 *     written at or past it, and nothing outside [ptr[j], ptr[j+1]) for any j.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed:
 *       < nunits          the first unit whose parse disagrees with its
 *                         offsets (as everywhere else);
 *       nunits + j        the first list j with ptr[j+1] < ptr[j] or
 *                         ptr[j+1] > out_values;
 *       nunits + nlists   the lists' unit counts do not add up to nunits.
 *     For either list-structure error the device decodes nothing and writes
 *     nothing to d_out.
 *   - TPF_EINVAL: a null d_in / d_off / d_list_ptr / d_out / d_ws, ws_bytes
 *     below tpf_p4ndec256v32_lists_workspace_size(nunits, nlists), nunits or
 *     nlists above 0x7FFFFFFF.  nlists == 0 or nunits == 0 is a successful
 *     no-op that still sets d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy (the structure is checked on the device), so the
 *     call sits inside a caller's pipeline like the other entries.  There is
 *     no limit on a list's length other than nunits.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_p4ndec256v32_lists_workspace_size(uint64_t nunits, uint64_t nlists);
int tpf_p4ndec256v32_lists(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                           const uint64_t *d_list_ptr, uint64_t nlists, int d1, const uint32_t *d_start0, uint32_t *d_out,
                           uint64_t out_values, void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* tpf_p4nenc256v32_lists is the mirror: it PRODUCES that stream from nlists
 * posting lists in ONE submission (replacing a loop of tpf_p4nenc256v32 calls,
 * or a gather into aligned copies around the batch encoders).  Its d_out,
 * d_off, d_list_ptr and d_start0 feed tpf_p4ndec256v32_lists unchanged.
 *   - Input (CSR form): d_list_ptr[0..nlists] is non-decreasing; list j is the
 *     n_j = ptr[j+1] - ptr[j] values at d_in + ptr[j], so the input is dense
 *     and ragged, positions only 4-byte aligned.  ptr[0] need not be 0.  Empty
 *     lists are allowed anywhere, any number in a row.  in_values is the
 *     readable length of d_in in values: nothing at or past it is read, and
 *     nothing outside [ptr[j], ptr[j+1]) for any j -- in particular never the
 *     value before a list.
 *   - Output: list j's stream is byte for byte what
 *     tpf_p4nenc256v32(d_in + ptr[j], n_j, d1, start0[j], ...) writes: its full
 *     p4{,D1}Enc256v32 blocks, then one p4{,D1}Enc32 block of n_j % 256 values;
 *     the lists concatenated in list order with no padding between them.
 *     d_off[0..nunits] receives the units' byte offsets: d_off[0] = 0 and
 *     d_off[nunits] is the stream's length.
 *   - Delta-1: with d1 != 0 the first unit of list j starts from d_start0[j]
 *     (the value before its first; d_start0 == NULL means 0 for every list),
 *     every later unit, the tail included, from the input value before it; a
 *     tail-only list's tail starts from d_start0[j].  Arithmetic is mod 2^32.
 *     With d1 == 0 d_start0 is ignored.
 *   - nunits is the capacity of d_off in units (nunits + 1 writable entries)
 *     and must equal the sum of units_j = n_j/256 + (n_j%256 != 0).
 *   - Capacity is checked on the device, once the sizes are known: when the
 *     stream is longer than out_cap nothing is written to d_out, but d_off is
 *     still filled completely and correctly, so d_off[nunits] tells the caller
 *     what to allocate.  Nothing is ever written at or past d_out + out_cap,
 *     nor before d_out.  tpf_p4nenc256v32_lists_bound(nvalues, nlists) is
 *     advice, a capacity that always suffices, not a precondition.  It sums the
 *     per-unit bounds of the batch encoders -- 1800 B per full block (at most
 *     8 B per value), 128 + 8 r B per tail of r values -- over the worst way
 *     nvalues values can fall into nlists lists: T = min(nlists, nvalues)
 *     tails, as few full blocks as the T tails (255 values each at most) leave,
 *         8 nvalues + 128 T - floor(248 max(0, nvalues - 255 T - 255) / 256) + 64
 *     (the block count taken without rounding up, which keeps the bound
 *     non-decreasing in both arguments).
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed:
 *       nunits + j          the first list j with ptr[j+1] < ptr[j] or
 *                           ptr[j+1] > in_values;
 *       nunits + nlists     the lists' unit counts do not add up to nunits;
 *       nunits + nlists + 1 out_cap is below the stream's length.
 *     For either list-structure error neither d_out nor d_off is written.  An
 *     encoder has no per-unit parse error: values < nunits are never reported.
 *   - TPF_EINVAL: a null d_list_ptr, d_off or d_ws when nlists is non-zero, a
 *     null d_in or d_out when nunits is non-zero, ws_bytes below
 *     tpf_p4nenc256v32_lists_workspace_size(nunits, nlists), nunits or nlists
 *     above 0x7FFFFFFF.  nlists == 0, or nunits == 0 with every list empty, is
 *     a successful no-op that sets d_off[0] = 0 and d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy, and a fixed number of launches whatever the number
 *     of lists and their lengths.
 * d_ws: device workspace, at least 8-byte aligned. */
uint64_t tpf_p4nenc256v32_lists_bound(uint64_t nvalues, uint64_t nlists);
size_t tpf_p4nenc256v32_lists_workspace_size(uint64_t nunits, uint64_t nlists);
int tpf_p4nenc256v32_lists(const uint32_t *d_in, uint64_t in_values, const uint64_t *d_list_ptr, uint64_t nlists, int d1,
                           const uint32_t *d_start0, uint8_t *d_out, uint64_t out_cap, uint64_t *d_off, uint64_t nunits,
                           void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- the read side of a resident index ---------------------------------------
 * A search engine keeps the stream of tpf_p4nenc256v32_lists resident and, for
 * each batch of queries, decodes the few lists the query terms name.
 *
 * tpf_lists_unit_base builds the UNIT DIRECTORY of a stream, once per index,
 * to be kept beside d_off and d_list_ptr: d_list_unit[j] is the index of the
 * first unit of list j -- the exclusive prefix sum of units_j = n_j/256 +
 * (n_j%256 != 0) -- and d_list_unit[nlists] the unit count of the stream.
 *   - Errors through d_err (optional; UINT64_MAX = clean): the first list j
 *     with ptr[j+1] < ptr[j] is reported as j, a unit total above 0x7FFFFFFF as
 *     nlists; in both cases nothing is written to d_list_unit.
 *   - TPF_EINVAL: a null d_list_unit; a null d_list_ptr or d_ws, or ws_bytes
 *     below tpf_lists_unit_base_workspace_size(nlists), when nlists is
 *     non-zero; nlists above 0x7FFFFFFF.  nlists == 0 writes d_list_unit[0] = 0.
 *   - Everything is enqueued on `stream`. */
size_t tpf_lists_unit_base_workspace_size(uint64_t nlists);
int tpf_lists_unit_base(const uint64_t *d_list_ptr, uint64_t nlists, uint32_t *d_list_unit /* nlists + 1 */, void *d_ws,
                        size_t ws_bytes, uint64_t *d_err, void *stream);

/* tpf_p4ndec256v32_lists_select decodes lists d_sel[0..nsel) of a resident
 * stream, in the order given, into one dense output, in ONE submission whose
 * cost depends on what is selected and not on the size of the index.
 *   - Output layout: selection k names list j = d_sel[k] of n_j = ptr[j+1] -
 *     ptr[j] values, written to d_out + d_out_ptr[k]; d_out_ptr[0] = 0 and
 *     d_out_ptr[k+1] = d_out_ptr[k] + n_j, so the output is dense, in selection
 *     order, and itself a CSR array (d_out_ptr: nsel + 1 entries, written).
 *     Only differences of d_list_ptr are used: its absolute values need not
 *     fit out_values.  The same list may be selected several times, each
 *     occurrence getting its own copy; empty lists may be selected, any number
 *     in a row.
 *   - Source units: the units of list j are d_list_unit[j] .. d_list_unit[j+1]
 *     of the stream (tpf_lists_unit_base), under the OFFSETS CONTRACT above.
 *   - Delta-1: with d1 != 0 the first unit of selection k starts from
 *     d_start0[d_sel[k]] -- d_start0 is indexed by the lists of the INDEX;
 *     NULL means 0 -- and every later unit, the tail included, from the
 *     decoded value before it, mod 2^32.  The results are exactly those of
 *     tpf_p4ndec256v32_lists.  With d1 == 0 d_start0 is ignored.
 *   - Output bounds: nothing is written at or past d_out + out_values, and
 *     nothing outside [d_out_ptr[k], d_out_ptr[k+1]) for any k.  d_out is only
 *     4-byte aligned.
 *   - Cost: no kernel is sized by nlists or nunits, and no pass reads d_off,
 *     d_in, d_list_ptr, d_list_unit or d_start0 at a list or unit that is not
 *     selected -- but for d_list_ptr[j+1], d_list_unit[j+1] and the end offset
 *     of a selected list's last unit.  Grids and the workspace are sized on
 *     the host from nsel and out_values alone: a selection that fits holds at
 *     most out_values/256 + nsel units (waves past the real count exit), so
 *     pass the capacity the selection needs, not the index's.  The number of
 *     launches is fixed, whatever the selection.  With d1 every selected full
 *     block is decoded twice (once for its sum, once for its values).
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed:
 *       < nunits        the SOURCE unit index of the first selected unit whose
 *                       parse disagrees with its offsets (the lowest such
 *                       index when several disagree);
 *       nunits + k      the first selection k with d_sel[k] >= nlists,
 *                       ptr[j+1] < ptr[j], d_list_unit[j+1] - d_list_unit[j]
 *                       different from the unit count of n_j, or
 *                       d_list_unit[j+1] > nunits: nothing is written to d_out
 *                       or d_out_ptr;
 *       nunits + nsel   the selected values do not fit out_values: nothing is
 *                       written to d_out, but d_out_ptr is filled completely,
 *                       so d_out_ptr[nsel] tells the caller what to allocate
 *                       (the rule tpf_p4nenc256v32_lists uses for out_cap).
 *   - TPF_EINVAL (decided before any device call): with nsel non-zero a null
 *     d_sel, d_out_ptr, d_in, d_off, d_list_ptr, d_list_unit, d_out or d_ws, or
 *     ws_bytes below tpf_p4ndec256v32_lists_select_workspace_size(nsel,
 *     out_values); nlists, nunits, nsel or out_values/256 + nsel above
 *     0x7FFFFFFF.  nsel == 0 is a successful no-op that writes d_out_ptr[0] = 0
 *     and sets d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_p4ndec256v32_lists_select_workspace_size(uint64_t nsel, uint64_t out_values);
int tpf_p4ndec256v32_lists_select(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                                  const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists, int d1,
                                  const uint32_t *d_start0, const uint32_t *d_sel, uint64_t nsel, uint32_t *d_out,
                                  uint64_t out_values, uint64_t *d_out_ptr /* nsel + 1 */, void *d_ws, size_t ws_bytes,
                                  uint64_t *d_err, void *stream);

/* ---- block-range reads of a resident index --------------------------------------
 * A conjunctive query pairs a short list with a long one and needs only the
 * few 256-value blocks of the long list whose doc-id range the short list
 * reaches.  The three entry points below add the SKIP TABLE every CPU user of
 * this codec keeps -- one uint32 per unit, the last value of that unit -- a
 * search from doc-id ranges to unit ranges over it, and a decode of unit ranges
 * of selected lists.  They compose on the device with no host step.
 *
 * tpf_lists_unit_last builds the skip table of a DELTA-1 lists stream, once per
 * index, to be kept beside d_off, d_list_ptr and d_list_unit.
 *   - Input: exactly what tpf_p4ndec256v32_lists takes with d1 != 0 (stream,
 *     offsets, CSR pointers, d_start0 or NULL for 0), minus the output array.
 *   - d_unit_last[u] (nunits entries, written) is the last decoded value of
 *     unit u, mod 2^32: for unit i of list j the value at position
 *     min(256 (i+1), n_j) - 1 of the list.  Tail units are included.
 *   - Errors through d_err (optional; UINT64_MAX = clean), as
 *     tpf_p4ndec256v32_lists reports them: < nunits the first unit whose parse
 *     disagrees with its offsets; nunits + j the first list j with ptr[j+1] <
 *     ptr[j]; nunits + nlists the lists' unit counts do not add up to nunits.
 *     There is no output array, so the pointers are not held against
 *     out_values.  On either list-structure error nothing is written to
 *     d_unit_last.
 *   - Cost: the index is read once and never decoded into a value-sized
 *     buffer; the workspace is O(nunits + nlists).  A fixed number of launches.
 *   - TPF_EINVAL (decided before any device call): nunits or nlists above
 *     0x7FFFFFFF; with both non-zero a null d_in, d_off, d_list_ptr,
 *     d_unit_last or d_ws, or ws_bytes below
 *     tpf_lists_unit_last_workspace_size(nunits, nlists).  nunits == 0 or
 *     nlists == 0 is a successful no-op that sets d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy. */
size_t tpf_lists_unit_last_workspace_size(uint64_t nunits, uint64_t nlists);
int tpf_lists_unit_last(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                        const uint64_t *d_list_ptr, uint64_t nlists, const uint32_t *d_start0,
                        uint32_t *d_unit_last /* nunits */, void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- opening a stream that has no offsets -------------------------------------
 * The reference writes no offsets, and an index built with it is a postings
 * file plus a term dictionary: per list a byte position and a count, nothing
 * per unit.  tpf_lists_unit_offsets rebuilds d_off[0..nunits] of such a stream
 * on the device from the lists' byte spans and the units' own headers, so that
 * with tpf_lists_unit_base and tpf_lists_unit_last every table of a resident
 * index can be rebuilt there.  Its sequential definition is
 * tpf_lists_scan_offsets (turbopfor_capi.h): the two agree offset for offset
 * and code for code.
 *   - Input: d_list_ptr (nlists + 1, non-decreasing; only differences are
 *     used: n_j = ptr[j+1] - ptr[j]) and d_list_byte (nlists + 1,
 *     non-decreasing, d_list_byte[nlists] <= in_bytes; d_list_byte[0] need not
 *     be 0).  List j's stream is exactly the bytes [d_list_byte[j],
 *     d_list_byte[j+1]) of d_in: n_j/256 p4Enc256v32 blocks and one p4Enc32
 *     tail of n_j%256 values.  Lists are contiguous, as every entry point
 *     above requires; an empty list has an empty span.  d_in may start at any
 *     byte address.
 *   - Output: d_off[d_list_unit[j] + i] is the byte offset of unit i of list j
 *     and d_off[nunits] = d_list_byte[nlists] (nunits + 1 entries, written).
 *     d_list_unit (optional, nlists + 1 entries) is what tpf_lists_unit_base
 *     writes.  The result feeds every lists entry point unchanged, on the same
 *     stream; for a stream written by tpf_p4nenc256v32_lists it is the
 *     encoder's d_off shifted by d_list_byte[0].
 *   - What is parsed: every unit's length, from its header bytes by the rules
 *     of tpf_block_size, refusals included (b > 32, bx > 32, a constant wider
 *     than 4 bytes in a tail, truncation), held to the rest of its list's
 *     span; the last unit of a list must end exactly at d_list_byte[j+1].  No
 *     base payload is read: headers, exception bitmaps and vbyte marker bytes
 *     only.
 *   - Bounds: nothing at or past d_in + in_bytes can change a result; the
 *     values of d_list_ptr and d_list_byte are checked, never followed; nothing
 *     is written outside d_off[0..nunits] and d_list_unit[0..nlists].
 *   - Errors through d_err (optional; UINT64_MAX = clean), the lowest code:
 *       < nunits        the lowest unit whose parsed length is 0 (malformed, or
 *                       past its list's span) or, for a list's last unit,
 *                       differs from what is left of the span.  Every other
 *                       list is complete and correct; in the offending list the
 *                       units after the bad one get d_list_byte[j+1], which is
 *                       in bounds and non-decreasing;
 *       nunits + j      the first list j with ptr[j+1] < ptr[j], byte[j+1] <
 *                       byte[j], byte[j+1] > in_bytes, or n_j == 0 with a
 *                       non-empty span: nothing is written;
 *       nunits + nlists the unit counts do not add up to nunits: nothing is
 *                       written.
 *   - TPF_EINVAL (decided before any device call): nunits or nlists above
 *     0x7FFFFFFF; a null d_off; with nlists non-zero a null d_list_ptr,
 *     d_list_byte or d_ws, or ws_bytes below
 *     tpf_lists_unit_offsets_workspace_size(nunits, nlists); a null d_in with
 *     nunits non-zero.  nlists == 0 is a successful no-op that writes d_off[0]
 *     = 0 and sets d_err to clean.
 *   - Workspace: under the WORKSPACE CONTRACT above (the export is a multiple
 *     of 256 and non-decreasing in both counts).
 *   - Cost: parallel across lists; inside a list the walk is a dependent chain
 *     of one step per unit, so the longest list sets a latency floor (DESIGN.md
 *     4.21).  A list of one unit needs no walk.
 *   - Everything is enqueued on `stream`: no host synchronisation, no
 *     device-to-host copy, a number of launches fixed by the arguments' sizes;
 *     the call can be captured into a hipGraph. */
size_t tpf_lists_unit_offsets_workspace_size(uint64_t nunits, uint64_t nlists);
int tpf_lists_unit_offsets(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_list_ptr,
                           const uint64_t *d_list_byte /* nlists + 1 */, uint64_t nlists, uint64_t *d_off /* nunits + 1 */,
                           uint64_t nunits, uint32_t *d_list_unit /* nlists + 1, optional */, void *d_ws, size_t ws_bytes,
                           uint64_t *d_err, void *stream);

/* tpf_lists_range_units answers nq range queries over the skip table: query k
 * asks for the units of list j = d_qlist[k] that can hold a value in
 * [d_qlo[k], d_qhi[k]], both ends inclusive.
 *   - With ua = d_list_unit[j] and ub = d_list_unit[j+1]: a is the first unit
 *     of [ua, ub) with d_unit_last >= lo, b the first with d_unit_last >= hi, or
 *     ub - 1 if there is none.  d_ufirst[k] = a - ua (list-relative) and
 *     d_ucount[k] = b - a + 1.  With no such a, with lo > hi, or for an empty
 *     list the result is (0, 0).  The named units are a superset of the units
 *     holding a value in range by at most one unit at the top end (the list's
 *     last unit when hi lies past the list).
 *   - Precondition: the list ascends without wrapping mod 2^32.  For a list
 *     that wraps, which units are named is unspecified, but the result still
 *     lies inside the list: d_ufirst + d_ucount <= ub - ua.
 *   - The outputs feed tpf_p4ndec256v32_lists_units unchanged, on the same
 *     stream: d_qlist as d_sel, d_ufirst and d_ucount as they are.
 *   - Errors through d_err (optional; UINT64_MAX = clean): the first query k
 *     with d_qlist[k] >= nlists, ub < ua or ub > nunits.  Such a query gets
 *     (0, 0) -- it decodes nothing -- and every other query is still answered.
 *     The values are checked, never followed.
 *   - One thread per query, two binary searches (12 dependent loads each for a
 *     list of 4,096 units); one launch, sized by nq alone.
 *   - TPF_EINVAL (decided before any device call): nlists, nunits or nq above
 *     0x7FFFFFFF; with nq non-zero a null d_list_unit, d_unit_last, d_qlist,
 *     d_qlo, d_qhi, d_ufirst or d_ucount.  nq == 0 is a successful no-op that
 *     sets d_err to clean.
 *   - Everything is enqueued on `stream`. */
int tpf_lists_range_units(const uint32_t *d_list_unit, const uint32_t *d_unit_last, uint64_t nlists, uint64_t nunits,
                          const uint32_t *d_qlist, const uint32_t *d_qlo, const uint32_t *d_qhi, uint64_t nq,
                          uint32_t *d_ufirst, uint32_t *d_ucount, uint64_t *d_err, void *stream);

/* tpf_p4ndec256v32_lists_units decodes unit ranges of selected lists of a
 * resident stream into one dense output: selection k names units
 * [d_ufirst[k], d_ufirst[k] + d_ucount[k]) of list j = d_sel[k], list-relative.
 *   - Lists may come in any order; the same list may repeat, with the same or
 *     different ranges, each occurrence getting its own copy; d_ucount[k] == 0
 *     is allowed anywhere, any number in a row.
 *   - Output layout: selection k yields 256 * ucount values, or
 *     256 * (ucount - 1) + n_j % 256 when the range reaches the list's p4Enc32
 *     tail unit, written to d_out + d_out_ptr[k]; d_out_ptr (nsel + 1 entries,
 *     written) is a CSR array starting at 0, so the output is dense and in
 *     selection order.  The value at list position p of a selected unit is bit
 *     for bit what tpf_p4ndec256v32_lists writes at ptr[j] + p.
 *   - Delta-1: with d1 != 0 d_unit_last (tpf_lists_unit_last) is required.
 *     Source unit su of list j starts from d_start0[j] (NULL means 0) when it is
 *     the list's first unit, else from d_unit_last[su - 1].  Every selected
 *     block is read and decoded ONCE: there is no sums pass, and the launch
 *     count is that of the plain form.  The table holds values, not indices: a
 *     wrong table gives wrong values and never an out-of-range access.  With
 *     d1 == 0 d_unit_last and d_start0 are ignored, so a frequency list stored
 *     in parallel is read over the unit ranges found for its doc-id list.
 *   - Output bounds: nothing is written at or past d_out + out_values, and
 *     nothing outside [d_out_ptr[k], d_out_ptr[k+1]) for any k.  d_out is only
 *     4-byte aligned.
 *   - Cost: as tpf_p4ndec256v32_lists_select.  No kernel is sized by nlists or
 *     nunits, and no pass reads the index at a unit that is not selected --
 *     but for d_list_ptr[j+1] and d_list_unit[j+1] of a selected list, the end
 *     offset of a selected unit, and with d1 d_unit_last of the unit before a
 *     selected one.  Grids and the workspace are sized on the host from nsel
 *     and out_values alone (a selection that fits holds at most
 *     out_values/256 + nsel units).  Ten launches (two of them reset d_err and
 *     the workspace header), whatever the selection, d1 or plain.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed:
 *       < nunits        the lowest SOURCE unit index among the selected units
 *                       whose parse disagrees with its offsets;
 *       nunits + k      the first selection k refused by any check of
 *                       tpf_p4ndec256v32_lists_select, or with d_ufirst[k] +
 *                       d_ucount[k] (summed without 32-bit wrap) above the unit
 *                       count of list j: nothing is written to d_out or
 *                       d_out_ptr;
 *       nunits + nsel   the selected values do not fit out_values: nothing is
 *                       written to d_out, but d_out_ptr is filled completely.
 *   - TPF_EINVAL (decided before any device call): with nsel non-zero a null
 *     d_sel, d_ufirst, d_ucount, d_out_ptr, d_in, d_off, d_list_ptr,
 *     d_list_unit, d_out or d_ws, a null d_unit_last when d1 != 0, or ws_bytes
 *     below tpf_p4ndec256v32_lists_units_workspace_size(nsel, out_values);
 *     nlists, nunits, nsel or out_values/256 + nsel above 0x7FFFFFFF.
 *     nsel == 0 is a successful no-op that writes d_out_ptr[0] = 0 and sets
 *     d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_p4ndec256v32_lists_units_workspace_size(uint64_t nsel, uint64_t out_values);
int tpf_p4ndec256v32_lists_units(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                                 const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists, int d1,
                                 const uint32_t *d_start0, const uint32_t *d_unit_last, const uint32_t *d_sel,
                                 const uint32_t *d_ufirst, const uint32_t *d_ucount, uint64_t nsel, uint32_t *d_out,
                                 uint64_t out_values, uint64_t *d_out_ptr /* nsel + 1 */, void *d_ws, size_t ws_bytes,
                                 uint64_t *d_err, void *stream);

/* ---- intersection with a resident index --------------------------------------
 * tpf_lists_intersect answers nq membership queries against a delta-1 lists
 * stream: query k is the probe values d_probe[d_probe_ptr[k] ..
 * d_probe_ptr[k+1]), tested against list j = d_qlist[k].  It returns the
 * values that are also in list j, with where they were found.  Only the blocks
 * a probe value lands in are decoded, and no decoded block is written to
 * memory.  A k-term AND is the call chained k-1 times on the device: d_out and
 * d_out_ptr of one call are d_probe and d_probe_ptr of the next.
 *   - The index: the stream, its offsets (OFFSETS CONTRACT), d_list_ptr and
 *     d_list_unit as tpf_p4ndec256v32_lists_units reads them with d1 != 0;
 *     d_start0 (NULL means 0); the skip table d_unit_last
 *     (tpf_lists_unit_last), required.
 *   - The probe: d_probe_ptr (nq + 1 entries) is non-decreasing and need not
 *     start at 0; probe_values is the readable length of d_probe, and nothing
 *     outside [d_probe_ptr[0], d_probe_ptr[nq]) is read.  Empty segments are
 *     allowed anywhere; the same list may be the target of many queries.
 *     d_out must not overlap d_probe.
 *   - Definition, per probe value v at index i of query k, with ua =
 *     d_list_unit[j] and ub = d_list_unit[j+1]: u is the first unit of
 *     [ua, ub) with d_unit_last[u] >= v; with no such unit v is a miss.  Unit u
 *     is decoded from d_start0[j] when u == ua, else from d_unit_last[u-1], as
 *     tpf_p4ndec256v32_lists_units decodes it.  v is a hit iff it equals one of
 *     the unit's decoded values, at index p of the unit.  The hits of query k
 *     go to d_out[d_out_ptr[k] .. d_out_ptr[k+1]) in probe order; d_out_pidx
 *     (optional) gets i, the index into d_probe; d_out_tpos (optional) gets the
 *     list-relative position 256 (u - ua) + p.  d_out_ptr[0] = 0: the output
 *     is dense and itself a CSR array.
 *   - For a list that ascends without wrapping mod 2^32, with a correct table,
 *     this is exactly "v is in list j" (the precondition of
 *     tpf_lists_range_units).  The probe need not be sorted or free of
 *     duplicates: the lookup is per value and every occurrence of a repeated
 *     value is reported.  A sorted probe makes the work minimal: a unit is
 *     decoded once per run of consecutive probe values that land in it.
 *   - Outside the precondition (a list that wraps, a wrong table) which members
 *     are reported is unspecified, but every reported triple is true of the
 *     decode -- the value at d_out_tpos, decoded from the table, equals v --
 *     and every access stays in bounds: the table holds values, never indices.
 *   - Output bounds: nothing is written at or past d_out + out_values (the same
 *     for d_out_pidx and d_out_tpos), and nothing outside a query's slice.
 *     d_out is only 4-byte aligned.  Hits never exceed the probe, so out_values
 *     = probe_values always suffices.
 *   - Cost: no kernel is sized by nlists or nunits.  Grids and the workspace
 *     (a few words per probe value) are sized on the host from probe_values
 *     alone.  Stream bytes are read only at units a probe value lands in;
 *     beyond them only the d_unit_last entries the searches visit and
 *     d_list_ptr, d_list_unit and d_start0 of targeted lists.  Ten launches
 *     for a probe of up to 262,144 values and twelve beyond (each of the two
 *     run scans then takes a second launch): decided on the host by
 *     probe_values, whatever the queries.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed:
 *       < nunits        the lowest SOURCE unit, among the units decoded, whose
 *                       parse disagrees with its offsets; hits of such a unit
 *                       are unspecified but in bounds;
 *       nunits + k      the first query k with d_qlist[k] >= nlists,
 *                       list_ptr[j+1] < list_ptr[j], list_unit[j+1] <
 *                       list_unit[j], list_unit[j+1] > nunits, a unit count
 *                       different from that of n_j, probe_ptr[k+1] <
 *                       probe_ptr[k] or probe_ptr[k+1] > probe_values: nothing
 *                       is written to d_out, d_out_ptr, d_out_pidx or
 *                       d_out_tpos;
 *       nunits + nq     the hits do not fit out_values: nothing is written to
 *                       d_out, d_out_pidx or d_out_tpos, but d_out_ptr is
 *                       filled completely, so d_out_ptr[nq] is what to allocate.
 *   - TPF_EINVAL (decided before any device call): with nq non-zero a null
 *     d_in, d_off, d_list_ptr, d_list_unit, d_unit_last, d_probe_ptr, d_qlist,
 *     d_out_ptr or d_ws; a null d_probe or d_out while probe_values or
 *     out_values is non-zero; ws_bytes below
 *     tpf_lists_intersect_workspace_size(nq, probe_values); nlists, nunits, nq
 *     or probe_values above 0x7FFFFFFF.  nq == 0 is a successful no-op that
 *     writes d_out_ptr[0] = 0 and sets d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_lists_intersect_workspace_size(uint64_t nq, uint64_t probe_values);
int tpf_lists_intersect(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                        const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists,
                        const uint32_t *d_start0, const uint32_t *d_unit_last,
                        const uint32_t *d_probe, uint64_t probe_values, const uint64_t *d_probe_ptr /* nq + 1 */,
                        const uint32_t *d_qlist, uint64_t nq,
                        uint32_t *d_out, uint64_t out_values, uint64_t *d_out_ptr /* nq + 1 */,
                        uint32_t *d_out_pidx /* optional */, uint32_t *d_out_tpos /* optional */,
                        void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- union with a resident index ----------------------------------------------
 * tpf_lists_union answers nq disjunctions against a delta-1 lists stream: query
 * k is the probe values d_probe[d_probe_ptr[k] .. d_probe_ptr[k+1]), merged
 * with list j = d_qlist[k].  It returns, per query, the sorted union of the two
 * with where every value came from.  A k-term OR is the call chained k-1 times
 * on the device: d_out and d_out_ptr of one call are d_probe and d_probe_ptr of
 * the next, and the first probe is a tpf_p4ndec256v32_lists_select decode.
 *   - The index and the probe: exactly the arguments of tpf_lists_intersect --
 *     the stream, its offsets, d_list_ptr, d_list_unit, d_start0 (NULL means
 *     0), the skip table d_unit_last (required); d_probe_ptr (nq + 1 entries)
 *     non-decreasing, not necessarily from 0; nothing of d_probe outside
 *     [d_probe_ptr[0], d_probe_ptr[nq]) is read.  Empty segments are allowed
 *     anywhere; the same list may be the target of many queries.  d_out must
 *     not overlap d_probe.
 *   - Definition.  Query k has target j = d_qlist[k] of n = n_j values, probe
 *     indices [a, b) = [d_probe_ptr[k], d_probe_ptr[k+1]), ua = d_list_unit[j]
 *     and ub = d_list_unit[j+1].  For probe index i with value v: u is the
 *     first unit of [ua, ub) with d_unit_last[u] >= v.  With no such unit L(i)
 *     = n and i is a MISS.  Otherwise unit u, of cnt values, is decoded as
 *     tpf_lists_intersect decodes it (from d_start0[j] when u == ua, else from
 *     d_unit_last[u-1]); q is the lower bound of v over the unit's decoded
 *     values by the intersection's branch-free search, held to cnt; L(i) =
 *     min(256 (u - ua) + q, n); i is a HIT iff q < cnt and the value at q
 *     equals v, else a miss.  M(i) is the number of misses among [a, i) and
 *     M_k the number of misses of the segment.
 *       Segment k of the output has n + M_k values at d_out[d_out_ptr[k] ..);
 *     d_out_ptr[0] = 0: the output is dense and itself a CSR array.
 *       Miss i goes to slot L(i) + M(i) of its segment; its d_out_pidx is i
 *     (the index into d_probe) and its d_out_tpos is TPF_LISTS_NONE.
 *       The list value at list position p goes to slot p + #{misses i' of the
 *     segment with L(i') <= p}; its d_out_tpos is p and its d_out_pidx is the
 *     probe index of the hit that equals it (the hit i with L(i) + M(i) = that
 *     slot), or TPF_LISTS_NONE.  The list's copy of a common value is the one
 *     kept: a hit adds no value.
 *   - Precondition: the list ascends without wrapping mod 2^32, the table is
 *     correct and the probe segment is strictly ascending.  Then segment k is
 *     exactly the sorted set union of the probe segment and the list, every
 *     slot written once, strictly ascending: a valid probe of the next call.
 *     Lists are limited to 2^32 - 1 values (d_out_tpos is 32 bits wide).
 *   - Outside the precondition (a list that wraps, a wrong table, an unsorted
 *     or repeating probe) d_out_ptr is still as defined, n + M_k per segment;
 *     the contents of the slices are unspecified; every access stays in
 *     bounds: the table holds values, never indices.
 *   - Output bounds: nothing is written at or past d_out + out_values (the same
 *     for d_out_pidx and d_out_tpos), and nothing outside a query's slice.
 *     d_out is only 4-byte aligned.  out_values = probe_values + the sum of the
 *     targets' lengths always suffices.
 *   - Cost: no kernel and no workspace array is sized by nlists or nunits.
 *     Grids and the workspace -- O(nq + probe_values + out_values / 256) words
 *     -- are sized on the host from nq, probe_values and out_values; a result
 *     that fits holds at most out_values / 256 + nq target units, the rule of
 *     tpf_p4ndec256v32_lists_select.  No decoded list value is staged in
 *     global memory.  A target unit is decoded at most twice: once if probe
 *     values land in it (the lookup), once when it is written.  Nineteen
 *     launches for a probe of up to 262,144 values and twenty-one beyond
 *     (each of the two run scans over the probe then takes a second launch),
 *     one fewer without d_out_pidx: decided on the host by the arguments'
 *     sizes, whatever the queries.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed, and the lowest code is the one reported:
 *       < nunits        the lowest SOURCE unit, among the units decoded, whose
 *                       parse disagrees with its offsets; the segment contents
 *                       are unspecified but in bounds;
 *       nunits + k      the first query k refused by any check
 *                       tpf_lists_intersect makes on a query: nothing is
 *                       written to d_out, d_out_ptr, d_out_pidx or d_out_tpos;
 *       nunits + nq     the result does not fit out_values: nothing is written
 *                       to d_out, d_out_pidx or d_out_tpos, but d_out_ptr is
 *                       filled completely, so d_out_ptr[nq] is what to allocate.
 *   - TPF_EINVAL (decided before any device call): with nq non-zero a null
 *     d_in, d_off, d_list_ptr, d_list_unit, d_unit_last, d_probe_ptr, d_qlist,
 *     d_out_ptr or d_ws; a null d_probe or d_out while probe_values or
 *     out_values is non-zero; ws_bytes below
 *     tpf_lists_union_workspace_size(nq, probe_values, out_values); nlists,
 *     nunits, nq, probe_values or out_values / 256 + nq above 0x7FFFFFFF.
 *     nq == 0 is a successful no-op that writes d_out_ptr[0] = 0 and sets d_err
 *     to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy.
 * d_ws: device workspace, at least 8-byte aligned. */
#define TPF_LISTS_NONE 0xFFFFFFFFu
size_t tpf_lists_union_workspace_size(uint64_t nq, uint64_t probe_values, uint64_t out_values);
int tpf_lists_union(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                    const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists,
                    const uint32_t *d_start0, const uint32_t *d_unit_last,
                    const uint32_t *d_probe, uint64_t probe_values, const uint64_t *d_probe_ptr /* nq + 1 */,
                    const uint32_t *d_qlist, uint64_t nq,
                    uint32_t *d_out, uint64_t out_values, uint64_t *d_out_ptr /* nq + 1 */,
                    uint32_t *d_out_pidx /* optional */, uint32_t *d_out_tpos /* optional */,
                    void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- difference with a resident index -----------------------------------------
 * tpf_lists_difference answers nq exclusions (AND NOT) against a delta-1 lists
 * stream: query k is the probe values d_probe[d_probe_ptr[k] ..
 * d_probe_ptr[k+1]), tested against list j = d_qlist[k].  It returns the values
 * that are NOT in list j, with where they would be inserted.  The argument list
 * is tpf_lists_intersect's, argument for argument: a caller switches operator
 * by switching the symbol.  "A AND NOT B AND NOT C" and the deleted-documents
 * filter ("result AND NOT tombstones") are the call chained on the device:
 * d_out and d_out_ptr of one call are d_probe and d_probe_ptr of the next.
 *   - The index and the probe: exactly the arguments of tpf_lists_intersect --
 *     the stream, its offsets, d_list_ptr, d_list_unit, d_start0 (NULL means
 *     0), the skip table d_unit_last (required); d_probe_ptr (nq + 1 entries)
 *     non-decreasing, not necessarily from 0; nothing of d_probe outside
 *     [d_probe_ptr[0], d_probe_ptr[nq]) is read.  Empty segments are allowed
 *     anywhere; the same list may be the target of many queries.  d_out must
 *     not overlap d_probe.
 *   - Definition: tpf_lists_union's.  Probe index i of query k, with value v
 *     and target j of n = n_j values, is a HIT or a MISS exactly as
 *     tpf_lists_union defines them, and L(i) is the union's: u is the first
 *     unit of [ua, ub) with d_unit_last[u] >= v; with no such unit L(i) = n and
 *     i is a miss; otherwise q is the branch-free lower bound of v over the
 *     decoded unit, held to cnt, L(i) = min(256 (u - ua) + q, n), and i is a
 *     hit iff q < cnt and the value at q equals v.
 *       The misses of query k go to d_out[d_out_ptr[k] .. d_out_ptr[k+1]) in
 *     probe order; d_out_ptr[0] = 0: the output is dense and itself a CSR
 *     array.  d_out_pidx (optional) gets i, the index into d_probe.
 *     d_out_tpos (optional) gets L(i): the number of list values below v,
 *     which is also the list position of the first value above v -- the
 *     advance(target) / next-doc-at-or-after answer of a posting-list cursor
 *     -- or n_j when there is none.  n_j is NOT a valid tpf_lists_gather
 *     position: drop such entries before reading successors.
 *   - The probe need not be sorted or free of duplicates, as with the
 *     intersection: the lookup is per value and every occurrence is reported.
 *     An ascending segment gives an ascending output segment, a valid probe of
 *     the next tpf_lists_intersect, tpf_lists_union or tpf_lists_difference.
 *   - Complement law.  On any input that passes the query checks and has no
 *     parse error, a probe index of [d_probe_ptr[0], d_probe_ptr[nq]) is
 *     reported by tpf_lists_difference iff tpf_lists_intersect on the same
 *     arguments does not report it: both use the same search.  So for a list
 *     that ascends without wrapping mod 2^32, with a correct table, this is
 *     exactly "v is not in list j".  Outside that precondition (a list that
 *     wraps, a wrong table) which indices are reported is unspecified, apart
 *     from the law itself, and every access stays in bounds: the table holds
 *     values, never indices.
 *   - Output bounds: nothing is written at or past d_out + out_values (the same
 *     for d_out_pidx and d_out_tpos), and nothing outside a query's slice.
 *     d_out is only 4-byte aligned.  Misses never exceed the probe, so
 *     out_values = probe_values always suffices.
 *   - Cost: no kernel and no workspace array is sized by nlists or nunits.
 *     Grids and the workspace (a few words per probe value; nq sizes nothing)
 *     are sized on the host from probe_values alone.  Stream bytes are read
 *     only at units a probe value lands in; a value past its list's last value,
 *     or aimed at an empty list, costs no decode.  d_list_ptr and d_list_unit
 *     are read by the plan as the intersection reads them, and again for
 *     misses only, when d_out_tpos is passed.  Ten launches for a probe of up
 *     to 262,144 values and twelve beyond (each of the two run scans then
 *     takes a second launch), two for nq == 0: decided on the host by
 *     probe_values, whatever the queries.
 *   - Errors through d_err (optional; UINT64_MAX = clean), the intersection's,
 *     code for code; the lowest code is the one reported:
 *       < nunits        the lowest SOURCE unit, among the units decoded, whose
 *                       parse disagrees with its offsets; which values of such
 *                       a unit are reported is unspecified but in bounds;
 *       nunits + k      the first query k refused by any check
 *                       tpf_lists_intersect makes on a query: nothing is
 *                       written to d_out, d_out_ptr, d_out_pidx or d_out_tpos;
 *       nunits + nq     the misses do not fit out_values: nothing is written to
 *                       d_out, d_out_pidx or d_out_tpos, but d_out_ptr is
 *                       filled completely, so d_out_ptr[nq] is what to allocate.
 *   - TPF_EINVAL (decided before any device call): with nq non-zero a null
 *     d_in, d_off, d_list_ptr, d_list_unit, d_unit_last, d_probe_ptr, d_qlist,
 *     d_out_ptr or d_ws; a null d_probe or d_out while probe_values or
 *     out_values is non-zero; ws_bytes below
 *     tpf_lists_difference_workspace_size(nq, probe_values); nlists, nunits, nq
 *     or probe_values above 0x7FFFFFFF.  nq == 0 is a successful no-op that
 *     writes d_out_ptr[0] = 0 and sets d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy; the call can be captured in a graph.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_lists_difference_workspace_size(uint64_t nq, uint64_t probe_values);
int tpf_lists_difference(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                         const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists,
                         const uint32_t *d_start0, const uint32_t *d_unit_last,
                         const uint32_t *d_probe, uint64_t probe_values, const uint64_t *d_probe_ptr /* nq + 1 */,
                         const uint32_t *d_qlist, uint64_t nq,
                         uint32_t *d_out, uint64_t out_values, uint64_t *d_out_ptr /* nq + 1 */,
                         uint32_t *d_out_pidx /* optional */, uint32_t *d_out_tpos /* optional */,
                         void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- values at list positions of a resident index -----------------------------
 * tpf_lists_gather answers nq positional reads against a lists stream, delta-1
 * or plain: query k is the positions d_pos[d_pos_ptr[k] .. d_pos_ptr[k+1]) of
 * list j = d_qlist[k], and d_out gets the value at each of them.  Only the
 * blocks a position names are decoded, and no decoded block is written to
 * memory.  It is what consumes d_out_tpos of tpf_lists_intersect: the term
 * frequencies of the hits are this call on the plain stream stored in parallel
 * with the doc-id stream; on a delta-1 stream it is "the doc id at rank p".
 *   - The index: the stream, its offsets (OFFSETS CONTRACT), d_list_ptr and
 *     d_list_unit as tpf_p4ndec256v32_lists_units reads them.  With d1 != 0 the
 *     skip table d_unit_last (tpf_lists_unit_last) is required and d_start0 ==
 *     NULL means 0; with d1 == 0 d_unit_last and d_start0 are ignored.  So the
 *     same d_list_ptr and d_list_unit serve a doc-id stream and the frequency
 *     stream of the same list lengths: only d_in, in_bytes, d_off and d1 differ.
 *   - The request: d_pos_ptr (nq + 1 entries) is non-decreasing and need not
 *     start at 0; pos_values is the readable length of d_pos and the writable
 *     length of d_out, and nothing of d_pos outside [d_pos_ptr[0],
 *     d_pos_ptr[nq]) is read.  Positions are list-relative, 0 <= p < n_j.
 *     Empty segments are allowed anywhere; the same list may be the target of
 *     many queries; positions may come in any order and may repeat, and every
 *     occurrence is answered.  Sorted positions make the work minimal: a unit
 *     is decoded once per run of consecutive request indices that name it, and
 *     an adjacent query on the same list and unit shares that run.
 *     d_out_tpos, d_out_ptr and d_qlist of a tpf_lists_intersect call feed this
 *     call unchanged, on the same stream, with no host step.
 *   - Definition, per request index i of query k, with p = d_pos[i]: the source
 *     unit is su = d_list_unit[j] + p / 256; with d1 it is decoded from
 *     d_start0[j] when it is the list's first unit, else from d_unit_last[su -
 *     1], as tpf_p4ndec256v32_lists_units decodes it.  d_out[i] is the value at
 *     index p % 256 of that unit: bit for bit what tpf_p4ndec256v32_lists
 *     writes at ptr[j] + p (with d1, given a correct table).  A wrong table
 *     gives wrong values and never an out-of-range access: the table holds
 *     values, never indices.
 *   - Output: d_out is parallel to d_pos -- the same index, so there is no
 *     compaction and no output pointer array.  Nothing is written outside
 *     [d_pos_ptr[0], d_pos_ptr[nq]).  d_out is only 4-byte aligned and must not
 *     overlap d_pos.
 *   - Cost: no kernel is sized by nlists or nunits.  Grids and the workspace
 *     (four words per position) are sized on the host from pos_values alone.
 *     Stream bytes are read only at units a position names; beyond them only
 *     d_list_ptr, d_list_unit and, with d1, d_start0 of targeted lists and
 *     d_unit_last of the unit before a named one.  Seven launches for up to
 *     262,144 positions and eight beyond (the run scan then takes a second
 *     launch): decided on the host by pos_values, whatever the request.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed:
 *       < nunits          the lowest SOURCE unit, among the units decoded,
 *                         whose parse disagrees with its offsets; values read
 *                         from such a unit are unspecified but in bounds;
 *       nunits + k        the first query k refused by any check
 *                         tpf_lists_intersect makes on a query: d_qlist[k] >=
 *                         nlists, list_ptr[j+1] < list_ptr[j], list_unit[j+1] <
 *                         list_unit[j], list_unit[j+1] > nunits, a unit count
 *                         different from that of n_j, pos_ptr[k+1] < pos_ptr[k]
 *                         or pos_ptr[k+1] > pos_values;
 *       nunits + nq + i   the lowest request index i, inside a segment of a
 *                         query that is not refused, with d_pos[i] >= n_j.
 *     On either refusal nothing is written to d_out; when both occur the query
 *     refusal (the lower code) is the one reported.
 *   - TPF_EINVAL (decided before any device call): with nq non-zero a null
 *     d_in, d_off, d_list_ptr, d_list_unit, d_pos_ptr, d_qlist or d_ws, or a
 *     null d_unit_last when d1 != 0; a null d_pos or d_out while pos_values is
 *     non-zero; ws_bytes below tpf_lists_gather_workspace_size(nq, pos_values);
 *     nlists, nunits, nq or pos_values above 0x7FFFFFFF.  nq == 0 is a
 *     successful no-op that sets d_err to clean.
 *   - Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_lists_gather_workspace_size(uint64_t nq, uint64_t pos_values);
int tpf_lists_gather(const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                     const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists, int d1,
                     const uint32_t *d_start0, const uint32_t *d_unit_last,
                     const uint32_t *d_pos, uint64_t pos_values, const uint64_t *d_pos_ptr /* nq + 1 */,
                     const uint32_t *d_qlist, uint64_t nq,
                     uint32_t *d_out /* pos_values entries, parallel to d_pos */,
                     void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- postings appended to a resident index ------------------------------------
 * tpf_lists_append extends the lists of a lists stream: list j of the result is
 * L_j ++ A_j, L_j being list j of the old index (empty for j >= nlists, which is
 * how new lists arrive) and A_j = d_add[d_add_ptr[j] .. d_add_ptr[j+1]).  A
 * 256v32 block's bytes depend on its 256 values and the value before it only,
 * so every full block of the old stream is moved as bytes; only the p4Enc32
 * tail of a list that receives values is decoded, joined with them and encoded
 * again.  Every table the readers need comes out of the same call: the result
 * feeds tpf_lists_intersect, tpf_lists_gather and tpf_p4ndec256v32_lists_units
 * with no further pass.  Appending to an empty index is encoding with the tables.
 *   - The old index: the stream, its offsets (OFFSETS CONTRACT), d_list_ptr and
 *     d_list_unit as tpf_p4ndec256v32_lists_units reads them; with d1 != 0 the
 *     skip table d_unit_last (tpf_lists_unit_last) is required.  d_start0 has
 *     nlists_out entries (NULL = 0; ignored with d1 == 0).  nlists == 0 or nunits
 *     == 0 is an empty old index: d_in, d_off, d_list_ptr and d_list_unit are
 *     then not read and may be NULL.
 *   - The additions: nlists_out >= nlists; d_add_ptr (nlists_out + 1 entries) is
 *     non-decreasing and need not start at 0; add_values is the readable length
 *     of d_add, and nothing of d_add outside [d_add_ptr[0], d_add_ptr[nlists_out])
 *     is read.  Empty additions and empty lists are allowed anywhere.
 *   - The result: d_list_ptr_out[0] = 0 and d_list_ptr_out[j+1] -
 *     d_list_ptr_out[j] = |L_j| + |A_j|; d_list_unit_out is what
 *     tpf_lists_unit_base gives for it, its last entry the result's unit count
 *     nunits_out.  For an old stream written by this library's encoders d_out and
 *     d_off_out[0 .. nunits_out] are byte for byte and offset for offset what
 *     tpf_p4nenc256v32_lists writes for the lists L_j ++ A_j with the same d1 and
 *     d_start0 (with d1: given a correct d_unit_last); for any old stream that
 *     passes the checks below the result decodes to L_j ++ A_j.  With d1,
 *     d_unit_last_out[0 .. nunits_out) is what tpf_lists_unit_last gives for the
 *     new stream.  The outputs must not overlap the inputs: the call is out of
 *     place and the caller swaps buffers.
 *   - What is read of the old stream, with r_j = |L_j| % 256: the |L_j| / 256
 *     full blocks of every list are copied and never parsed; the tail is parsed
 *     only when r_j > 0 and |A_j| > 0, and copied otherwise.  Interior offsets of
 *     copied units are carried over shifted and not checked; the ends of each
 *     copied byte range are.  With d1 the first re-encoded block of list j
 *     starts from d_start0[j] when |L_j| < 256, else from d_unit_last of the
 *     list's last full unit.  The table holds values, never indices: a wrong
 *     table gives wrong bytes and never an out-of-range access.
 *   - Capacities: units_cap is the capacity of d_off_out (units_cap + 1 entries)
 *     and of d_unit_last_out.  tpf_lists_append_units_bound = nunits + add_values
 *     / 256 + min(nlists_out, add_values) always suffices (ceil((a + m) / 256) <=
 *     ceil(a / 256) + m / 256 + 1 for m > 0), and so does tpf_lists_append_bound
 *     = in_bytes + tpf_p4nenc256v32_lists_bound(add_values + 255 T, T), T =
 *     min(nlists_out, add_values), for out_cap.  Both are advice, not
 *     preconditions: nothing is written at or past a capacity.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed; the lowest code is the one reported:
 *       < nunits                  the lowest old tail unit, among those parsed,
 *                                 whose parse disagrees with its offsets; what is
 *                                 written is unspecified but in bounds;
 *       nunits + j                the first list j < nlists_out that fails a
 *                                 structure check: list_ptr[j+1] < list_ptr[j]; a
 *                                 d_list_unit span different from the unit count
 *                                 of |L_j|; list_unit[j+1] > nunits; a copied byte
 *                                 range with off[lo] > off[hi] or off[hi] >
 *                                 in_bytes; add_ptr[j+1] < add_ptr[j]; add_ptr[j+1]
 *                                 > add_values.  Nothing is written, in any output;
 *       nunits + nlists_out       nunits_out > units_cap, or above 0x7FFFFFFF: only
 *                                 d_list_ptr_out and d_list_unit_out are written,
 *                                 completely, so the caller reads what to allocate;
 *       nunits + nlists_out + 1   the stream is longer than out_cap: everything
 *                                 is written except d_out, so
 *                                 d_off_out[nunits_out] is what to allocate.
 *   - TPF_EINVAL (decided before any device call): nlists_out < nlists; with
 *     nlists_out non-zero a null d_add_ptr, d_out (with out_cap non-zero),
 *     d_off_out, d_list_ptr_out, d_list_unit_out or d_ws, a null d_in, d_off,
 *     d_list_ptr or d_list_unit with nlists and nunits non-zero, a null
 *     d_unit_last or d_unit_last_out when d1 != 0, a null d_add while add_values
 *     is non-zero; ws_bytes below tpf_lists_append_workspace_size(nunits,
 *     nlists_out, add_values); nunits, nlists_out, units_cap or add_values above
 *     0x7FFFFFFF.  nlists_out == 0 is a successful no-op that writes
 *     d_list_ptr_out[0] = 0, d_list_unit_out[0] = 0, d_off_out[0] = 0 and a
 *     clean d_err.
 *   - Cost: the stitch pass moves the whole index once, partitioned by output
 *     bytes (16,384 per wave), not by list; everything else is sized by
 *     nlists_out, add_values and units_cap.  The workspace holds the staged
 *     values (add_values + 255 min(T, nunits)), their encoded bytes and the
 *     encoder's workspace.  Everything is enqueued on `stream`: no host
 *     synchronisation and no device-to-host copy; at most 23 launches, their
 *     number and their grids fixed by the arguments' sizes, not their contents.
 * d_ws: device workspace, at least 8-byte aligned. */
uint64_t tpf_lists_append_units_bound(uint64_t nunits, uint64_t nlists_out, uint64_t add_values);
uint64_t tpf_lists_append_bound(uint64_t in_bytes, uint64_t nlists_out, uint64_t add_values);
size_t   tpf_lists_append_workspace_size(uint64_t nunits, uint64_t nlists_out, uint64_t add_values);
int tpf_lists_append(
    /* the old index */   const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                          const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists,
                          int d1, const uint32_t *d_start0 /* nlists_out entries, or NULL = 0 */,
                          const uint32_t *d_unit_last /* required when d1 != 0 */,
    /* the additions */   const uint32_t *d_add, uint64_t add_values, const uint64_t *d_add_ptr /* nlists_out + 1 */,
                          uint64_t nlists_out,
    /* the new index */   uint8_t *d_out, uint64_t out_cap, uint64_t *d_off_out /* units_cap + 1 */, uint64_t units_cap,
                          uint64_t *d_list_ptr_out /* nlists_out + 1 */, uint32_t *d_list_unit_out /* nlists_out + 1 */,
                          uint32_t *d_unit_last_out /* units_cap; required when d1 != 0, ignored otherwise */,
                          void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- postings deleted from a resident index -----------------------------------
 * tpf_lists_remove shortens the lists of a lists stream: list j of the result is
 * L_j without the values at the list-relative positions a query names.  Every
 * unit of a list before the one that holds its first removed position keeps its
 * bytes, and so does every list that loses nothing; only the suffix of a list
 * from that unit on is decoded, compacted and encoded again.  Positions, not doc
 * ids: the same removals delete from a doc-id stream (d1 != 0) and from the
 * frequency stream stored in parallel over the same directory (d1 == 0).  Every
 * table the readers need comes out of the same call, as with tpf_lists_append.
 *   - The old index: as tpf_lists_append reads it; with d1 != 0 the skip table
 *     d_unit_last is required.  d_start0 has nlists entries (NULL = 0; ignored
 *     with d1 == 0).  With nunits == 0 d_in and d_off are not read.
 *   - The removals: segment k is d_pos[d_pos_ptr[k] .. d_pos_ptr[k+1]) and names
 *     positions of list d_qlist[k], strictly ascending within the segment.
 *     d_qlist is strictly ascending, so a list is targeted at most once.
 *     d_pos_ptr (nq + 1 entries) is non-decreasing and need not start at 0;
 *     pos_values is the readable length of d_pos and nothing of d_pos outside
 *     [d_pos_ptr[0], d_pos_ptr[nq]) is read.  Empty segments are allowed
 *     anywhere.  d_out_tpos, d_out_ptr and d_qlist of a tpf_lists_intersect call
 *     whose queries ascend by list and whose probe segments ascend feed the call
 *     unchanged.
 *   - The result: list ids are stable -- a list that loses everything stays, as
 *     an empty list.  d_list_ptr_out[0] = 0; d_list_unit_out is what
 *     tpf_lists_unit_base gives for the new lengths, its last entry the result's
 *     unit count nunits_out.  For an old stream written by this library's
 *     encoders d_out and d_off_out[0 .. nunits_out] are byte for byte and offset
 *     for offset what tpf_p4nenc256v32_lists writes for the shortened lists with
 *     the same d1 and d_start0 (with d1: given a correct d_unit_last).  With d1,
 *     d_unit_last_out[0 .. nunits_out) is what tpf_lists_unit_last gives for the
 *     new stream.  The outputs must not overlap the inputs: the call is out of
 *     place and the caller swaps buffers.
 *   - What is read of the old stream: for a targeted list with a non-empty
 *     segment and first removed position p0, u0 = p0 / 256.  Units [0, u0) of the
 *     list are copied and never parsed; units [u0, end) are decoded, from
 *     d_start0[j] when u0 == 0, else from d_unit_last of unit u0 - 1.  A list
 *     with no removals, its tail included, is copied and never parsed.  Interior
 *     offsets of copied ranges are carried over shifted and not checked; the ends
 *     of each copied byte range are held against in_bytes.  The table holds
 *     values, never indices: a wrong table gives wrong bytes and never an
 *     out-of-range access.
 *   - Staging: the call stages s_j = |L_j| - 256 u0 values per affected list and
 *     stage_values is the capacity of their sum.  The sum of |L_j| over the
 *     targeted lists always suffices.  The workspace, the decode and the encoder
 *     are sized by nq and stage_values, the per-list arrays by nlists; only the
 *     stitch pass and the offsets pass are sized by the whole index.
 *   - Capacities: units_cap is the capacity of d_off_out (units_cap + 1 entries)
 *     and of d_unit_last_out; nunits_out <= nunits always, so units_cap = nunits
 *     suffices.  The stream can grow (the merge of two deltas can widen a
 *     block): tpf_lists_remove_bound = in_bytes +
 *     tpf_p4nenc256v32_lists_bound(stage_values, nq) always suffices for out_cap.
 *     Both are advice, not preconditions: nothing is written at or past a
 *     capacity.
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed; the lowest code is the one reported:
 *       < nunits                  the lowest decoded unit whose offsets lie outside
 *                                 the stream or whose parse disagrees with them;
 *                                 what is written is unspecified but in bounds;
 *       nunits + j                the first list j that fails a structure check:
 *                                 list_ptr[j+1] < list_ptr[j]; a d_list_unit span
 *                                 different from the unit count of |L_j|;
 *                                 list_unit[j+1] > nunits; a copied byte range with
 *                                 off[lo] > off[hi] or off[hi] > in_bytes.  Nothing
 *                                 is written, in any output;
 *       nunits + nlists + k       the first refused query k: d_qlist[k] >= nlists;
 *                                 d_qlist[k] <= d_qlist[k-1]; pos_ptr[k+1] <
 *                                 pos_ptr[k]; pos_ptr[k+1] > pos_values; a position
 *                                 >= |L_j|; a position not above the one before it
 *                                 in its segment.  Nothing is written;
 *       nunits + nlists + nq      the staged values exceed stage_values: only
 *                                 d_list_ptr_out and d_list_unit_out are written,
 *                                 completely;
 *       nunits + nlists + nq + 1  nunits_out > units_cap: the two directories only;
 *       nunits + nlists + nq + 2  the stream is longer than out_cap: everything
 *                                 is written except d_out, so
 *                                 d_off_out[nunits_out] is what to allocate.
 *   - TPF_EINVAL (decided before any device call): a null d_off_out,
 *     d_list_ptr_out or d_list_unit_out; with nlists non-zero a null d_list_ptr,
 *     d_list_unit, d_ws or d_out (with out_cap non-zero), a null d_in or d_off
 *     with nunits non-zero, a null d_unit_last (with nunits non-zero) or
 *     d_unit_last_out when d1 != 0, a null d_pos_ptr or d_qlist with nq non-zero,
 *     a null d_pos with nq and pos_values non-zero; ws_bytes below
 *     tpf_lists_remove_workspace_size(nunits, nlists, nq, pos_values,
 *     stage_values); nunits, nlists, nq, pos_values, stage_values, units_cap or
 *     stage_values / 256 + nq + 1 above 0x7FFFFFFF.  nlists == 0 is a successful
 *     no-op that writes d_list_ptr_out[0] = 0, d_list_unit_out[0] = 0,
 *     d_off_out[0] = 0 and a clean d_err; nq == 0 with nlists != 0 is a plain
 *     restitch of the index.
 *   - Cost: the stitch pass moves the whole index once, as the append's.
 *     Everything is enqueued on `stream`: no host synchronisation and no
 *     device-to-host copy; at most 36 launches, their number and their grids
 *     fixed by the arguments' sizes, not their contents.
 * d_ws: device workspace, at least 8-byte aligned. */
uint64_t tpf_lists_remove_bound(uint64_t in_bytes, uint64_t nq, uint64_t stage_values);
size_t   tpf_lists_remove_workspace_size(uint64_t nunits, uint64_t nlists, uint64_t nq,
                                         uint64_t pos_values, uint64_t stage_values);
int tpf_lists_remove(
    /* the old index */ const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                        const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists,
                        int d1, const uint32_t *d_start0 /* nlists, or NULL = 0 */,
                        const uint32_t *d_unit_last /* required when d1 != 0 */,
    /* the removals */  const uint32_t *d_pos, uint64_t pos_values, const uint64_t *d_pos_ptr /* nq + 1 */,
                        const uint32_t *d_qlist /* nq */, uint64_t nq, uint64_t stage_values,
    /* the new index */ uint8_t *d_out, uint64_t out_cap, uint64_t *d_off_out /* units_cap + 1 */, uint64_t units_cap,
                        uint64_t *d_list_ptr_out /* nlists + 1 */, uint32_t *d_list_unit_out /* nlists + 1 */,
                        uint32_t *d_unit_last_out /* units_cap; required when d1 != 0 */,
                        void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- a sub-index of a resident index -------------------------------------------
 * tpf_lists_extract takes a lists stream apart: list k of the result is a unit
 * range of list d_sel[k] of the index, and the result is an index of its own --
 * stream, unit offsets, both directories, the delta-1 starts and the skip table
 * out of one call.  A unit's bytes depend on its values and the value before it
 * only, so a unit range of a list is the encoder's own stream for the values of
 * that range: the bytes are moved, nothing is parsed, decoded or encoded.  A
 * term shard (the lists with j % world == rank), a doc-id window (the ranges of
 * tpf_lists_range_units), the lists that stay resident after an eviction and the
 * part of an index that is saved or shipped are each one call.
 *   - The index: as tpf_p4ndec256v32_lists_units reads it.  d_start0 has nlists
 *     entries (NULL = 0).  With d1 == 0, d_start0, d_unit_last, d_start0_out and
 *     d_unit_last_out are ignored.  With nunits == 0 d_in and d_off are not read.
 *   - The selection: list k of the result is units [d_ufirst[k], d_ufirst[k] +
 *     d_ucount[k]) of list j = d_sel[k], list-relative; with d_ufirst == NULL it
 *     is all of list j and d_ucount is not read.  These are the arguments of
 *     tpf_p4ndec256v32_lists_units: d_qlist, d_ufirst and d_ucount of
 *     tpf_lists_range_units feed the call unchanged, on the same stream.
 *     Selections come in any order and may repeat; each occurrence gets a copy of
 *     its own.  Empty lists and d_ucount[k] == 0 are allowed anywhere, any number
 *     in a row, d_ufirst[k] == the list's unit count with a zero count included.
 *   - The result: list k has 256 * ucount values, or 256 * (ucount - 1) + n_j %
 *     256 when the range reaches the list's tail unit.  d_list_ptr_out[0] = 0;
 *     d_list_unit_out is what tpf_lists_unit_base gives for the result, its last
 *     entry the result's unit count nunits_out.  A unit range is a well-formed
 *     list: full blocks, then the tail at most once, at the end.
 *   - Delta-1 starts: d_start0_out[k] = d_start0[j] (0 for NULL) when the range
 *     starts the list (d_ufirst[k] == 0 or d_ufirst == NULL), else the skip
 *     table's entry of the unit before it, d_unit_last[d_list_unit[j] +
 *     d_ufirst[k] - 1].  d_unit_last is therefore required when d1 != 0 and
 *     d_ufirst != NULL and optional otherwise.  d_unit_last_out is written
 *     exactly when d1 != 0 and both d_unit_last and d_unit_last_out are non-null:
 *     the source entries of the copied units, which is what tpf_lists_unit_last
 *     gives for the new stream.  The frequency stream stored in parallel over
 *     the same directory is extracted by the same selection with d1 == 0.
 *   - Bytes: d_out is the selected units' bytes laid end to end in selection
 *     order, d_off_out[u] = (first output byte of list k) + d_off[src(u)] -
 *     d_off[src of k's first unit], d_off_out[0] = 0 and d_off_out[nunits_out]
 *     the stream's length.  For an index written by this library's encoders
 *     d_out and d_off_out are byte for byte and offset for offset what
 *     tpf_p4nenc256v32_lists writes for the selected values with d1 and
 *     d_start0_out; for any stream that passes the checks the result decodes to
 *     the selected values.  Interior offsets are carried over shifted and not
 *     checked; the two ends of each copied range are held against each other and
 *     against in_bytes.  The table holds values, never indices: a wrong table
 *     gives wrong starts and never an out-of-range access.  The outputs must not
 *     overlap the inputs.
 *   - Capacities: units_cap is the capacity of d_off_out (units_cap + 1 entries)
 *     and of d_unit_last_out, out_cap that of d_out.  Nothing is written at or
 *     past a capacity.  With repeats the result can be larger than the index, so
 *     there is no bound from the sizes alone: a call with out_cap == 0 and d_out
 *     == NULL is the sizing call (the last code below).
 *   - Errors through d_err (optional; UINT64_MAX = clean); the values are
 *     checked, never followed; the lowest code is the one reported.  Nothing is
 *     parsed, so no code below nunits is ever reported:
 *       nunits + k         the first refused selection k: d_sel[k] >= nlists;
 *                          list_ptr[j+1] < list_ptr[j]; a d_list_unit span
 *                          different from the unit count of n_j; list_unit[j+1] >
 *                          nunits; ufirst + ucount (summed without 32-bit wrap)
 *                          above the list's unit count; a copied byte range with
 *                          off[lo] > off[hi] or off[hi] > in_bytes.  Nothing is
 *                          written, in any output;
 *       nunits + nsel      nunits_out > units_cap or nunits_out > 0x7FFFFFFF:
 *                          only d_list_ptr_out, d_list_unit_out and, with d1,
 *                          d_start0_out are written, completely;
 *       nunits + nsel + 1  the stream is longer than out_cap: everything is
 *                          written except d_out, so d_off_out[nunits_out] is
 *                          what to allocate.
 *   - TPF_EINVAL (decided before any device call): a null d_off_out,
 *     d_list_ptr_out or d_list_unit_out; with nsel non-zero a null d_sel,
 *     d_list_ptr, d_list_unit or d_ws, a null d_out with out_cap non-zero, a null
 *     d_in or d_off with nunits non-zero, a null d_ucount with d_ufirst non-null,
 *     a null d_start0_out with d1 != 0, a null d_unit_last with d1 != 0 and
 *     d_ufirst non-null; ws_bytes below tpf_lists_extract_workspace_size(nsel);
 *     nunits, nlists, nsel or units_cap above 0x7FFFFFFF.  nsel == 0 is a
 *     successful no-op that writes d_list_ptr_out[0] = 0, d_list_unit_out[0] = 0,
 *     d_off_out[0] = 0 and a clean d_err.
 *   - Workspace: O(nsel), under the WORKSPACE CONTRACT above (the export is a
 *     multiple of 256 and non-decreasing in nsel).
 *   - Cost: no kernel is sized by nlists, nunits or in_bytes.  The plan and the
 *     workspace are sized by nsel, the offsets pass by units_cap and the move by
 *     out_cap, on the host; waves past the real totals exit.  Nothing of the
 *     index is read at a list or unit that is not selected, but for the [j+1]
 *     directory entries, the end offset of a selected range and, with d1,
 *     d_unit_last of the unit before a range.  Everything is enqueued on
 *     `stream`: no host synchronisation and no device-to-host copy, so the call
 *     can be captured into a hipGraph; 12 launches at the most (d_err's reset,
 *     the header's, the plan, 3 x 2 run scans, the heads, the offsets unless
 *     units_cap == 0, the move unless out_cap == 0; two with nsel == 0), their
 *     number and their grids fixed by the arguments' sizes, not their contents.
 * d_ws: device workspace, at least 8-byte aligned. */
size_t tpf_lists_extract_workspace_size(uint64_t nsel);
int tpf_lists_extract(
    /* the index */     const uint8_t *d_in, uint64_t in_bytes, const uint64_t *d_off, uint64_t nunits,
                        const uint64_t *d_list_ptr, const uint32_t *d_list_unit, uint64_t nlists,
                        int d1, const uint32_t *d_start0 /* nlists, or NULL = 0 */, const uint32_t *d_unit_last,
    /* the selection */ const uint32_t *d_sel, const uint32_t *d_ufirst /* NULL: whole lists */,
                        const uint32_t *d_ucount /* read only with d_ufirst */, uint64_t nsel,
    /* the new index */ uint8_t *d_out, uint64_t out_cap, uint64_t *d_off_out /* units_cap + 1 */, uint64_t units_cap,
                        uint64_t *d_list_ptr_out /* nsel + 1 */, uint32_t *d_list_unit_out /* nsel + 1 */,
                        uint32_t *d_start0_out /* nsel; required when d1 != 0 */,
                        uint32_t *d_unit_last_out /* units_cap; optional */,
                        void *d_ws, size_t ws_bytes, uint64_t *d_err, void *stream);

/* ---- host pipeline utility ----------------------------------------------
 * Copies `bytes` bytes with a kernel (16-byte non-temporal stores) instead of
 * an SDMA engine; either side may be pinned/registered host memory, at any
 * byte alignment.  The tpf_host_* pipelines use it for downloads under
 * TPF_HOST_DOWN=kernel (SDMA is their default: faster on MI355X). */
int tpf_copy_async(void *dst, const void *src, uint64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
