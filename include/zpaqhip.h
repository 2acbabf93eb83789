/* include/zpaqhip.h — C ABI of libzpaqhip.so: MI355X (gfx950) ZPAQ block decompression.
 *
 * This is the drop-in boundary for the reference's decompression path.  The
 * reference (mnadareski/ZPAQSharp) has no FFI layer of its own — the path is a
 * plain class API (Decompresser.cs:11-221 driven by LibZPAQ.decompress,
 * LibZPAQ.cs:65-79).  A maintainer binds these entry points with
 * [DllImport("zpaqhip", CallingConvention = CallingConvention.Cdecl)] and keeps
 * the Reader/Writer-facing classes unchanged; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C types only; no exceptions, exit() or longjmp cross the boundary;
 *   - every function returns 0 (ZPAQHIP_OK) or a negative zpaqhip_status; the
 *     codes map 1:1 onto the reference's error() messages (zpaqhip_strerror);
 *   - the library never keeps a caller pointer after a call returns;
 *   - a zpaqhip_ctx is bound to one GPU and is not thread-safe; distinct
 *     contexts are independent (libzpaq contract, reference LICENSE:44-46);
 *   - there is NO CPU decode path in this library: without a usable HIP device
 *     zpaqhip_ctx_create fails with ZPAQHIP_E_NO_DEVICE.
 */
#ifndef ZPAQHIP_H
#define ZPAQHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZPAQHIP_ABI_VERSION 1

typedef enum zpaqhip_status {
  ZPAQHIP_OK = 0,
  /* Decoder.cs */
  ZPAQHIP_E_CORRUPT = -1,        /* "archive corrupted"               Decoder.cs:141 */
  ZPAQHIP_E_EOF = -2,            /* "unexpected end of file"          Decoder.cs:154 */
  ZPAQHIP_E_EOS = -3,            /* "decoding end of stream"          Decoder.cs:43  */
  /* ZPAQL.cs */
  ZPAQHIP_E_ZPAQL = -4,          /* "ZPAQL execution error"           ZPAQL.cs:1314-1317 */
  ZPAQHIP_E_HEADER = -5,         /* header errors                     ZPAQL.cs:128-148 */
  ZPAQHIP_E_HM_TOO_BIG = -6,     /* "H too big" / "M too big"         ZPAQL.cs:1021-1022 */
  /* Predictor.cs:100-166 component limit checks */
  ZPAQHIP_E_COMPONENT = -7,
  /* PostProcessor.cs */
  ZPAQHIP_E_PP_EOS = -8,         /* "Unexpected EOS"                  PostProcessor.cs:43,52,57,68 */
  ZPAQHIP_E_PP_TYPE = -9,        /* "unknown post processing type"    PostProcessor.cs:45 */
  ZPAQHIP_E_PP_EMPTY = -10,      /* "Empty PCOMP"                     PostProcessor.cs:59 */
  /* Decompresser.cs framing */
  ZPAQHIP_E_LEVEL = -11,         /* "unsupported ZPAQ level"/"ZPAQL type" Decompresser.cs:49-50 */
  ZPAQHIP_E_SEGMENT = -12,       /* "missing segment or end of block" Decompresser.cs:90 */
  ZPAQHIP_E_FRAMING_EOF = -13,   /* "unexpected EOF"                  Decompresser.cs:77,103 */
  ZPAQHIP_E_RESERVED = -14,      /* "missing reserved byte"           Decompresser.cs:107 */
  ZPAQHIP_E_SEGEND = -15,        /* "missing end of segment marker"   Decompresser.cs:193 */
  /* build-specific */
  ZPAQHIP_E_OUTPUT_FULL = -20,   /* caller's output buffer too small (out_len still reports the need) */
  ZPAQHIP_E_SHA1 = -21,          /* stored SHA-1 does not match decoded segment */
  ZPAQHIP_E_NO_DEVICE = -22,     /* no usable HIP device / kernels not loadable */
  ZPAQHIP_E_DEVICE_MEM = -23,    /* model does not fit device memory ("Out of memory") */
  ZPAQHIP_E_HIP = -24,           /* HIP runtime error (message in zpaqhip_err) */
  ZPAQHIP_E_ARG = -25,           /* bad argument / table too small */
  ZPAQHIP_E_BUDGET = -26,        /* ZPAQL instruction budget exhausted (runaway program guard) */
  ZPAQHIP_E_CALLBACK = -27,      /* read/write callback failed */
  ZPAQHIP_E_VERIFY = -28         /* "Pre/post-processor test failed"  LibZPAQ.cs:320 */
} zpaqhip_status;

typedef struct zpaqhip_err {
  int32_t code;        /* zpaqhip_status */
  int32_t block;       /* block index the error belongs to, or -1 */
  int32_t segment;     /* segment index (global), or -1 */
  char msg[116];       /* NUL-terminated English message (reference wording) */
} zpaqhip_err;

/* One block of the stream, as located by zpaqhip_scan (Decompresser.findBlock,
 * Decompresser.cs:29-58 + ZPAQL.read, ZPAQL.cs:112-156). */
typedef struct zpaqhip_block {
  uint64_t tag_off;      /* offset of the 13-byte tag + "zPQ" locator (start of the 16-byte string) */
  uint64_t hdr_off;      /* offset of the header (hsize low byte) */
  uint32_t hdr_len;      /* hsize + 2 */
  uint8_t level;         /* 1 or 2 */
  uint8_t n_comp;        /* header[6] */
  uint8_t hh, hm, ph, pm;
  uint16_t reserved;
  uint32_t first_seg;    /* index into the segment table */
  uint32_t n_seg;
  uint64_t end_off;      /* offset just past the block's 255 terminator */
  double model_mem;      /* ZPAQL.memory(), ZPAQL.cs:58-81 */
  uint64_t usize_hint;   /* sum of decimal sizes in the segment comments, or UINT64_MAX */
} zpaqhip_block;

/* One segment (Decompresser.findFilename/readComment/readSegmentEnd,
 * Decompresser.cs:67-108,163-194). */
typedef struct zpaqhip_segment {
  uint32_t block;        /* owning block */
  uint32_t flags;        /* bit0: SHA-1 present */
  uint64_t name_off;     /* filename bytes [name_off, name_off+name_len) */
  uint32_t name_len;
  uint32_t comment_len;
  uint64_t comment_off;
  uint64_t data_off;     /* first coded byte */
  uint64_t data_len;     /* coded bytes incl. the 4 zero bytes that end the segment */
  uint64_t usize_hint;   /* decimal size from the comment, or UINT64_MAX */
  uint8_t sha1[20];      /* stored checksum if flags&1 */
  uint32_t reserved;
} zpaqhip_segment;

/* Per-segment result of a decode. */
typedef struct zpaqhip_seg_result {
  int32_t status;        /* zpaqhip_status */
  uint32_t pp_state;     /* PostProcessor state at the end (1 PASS, 5 PROG) */
  uint64_t out_off;      /* where the segment's plaintext starts in the output */
  uint64_t out_len;      /* plaintext bytes produced (counted even past capacity) */
  uint64_t in_used;      /* coded bytes the decoder consumed; != data_len means the stream is damaged */
} zpaqhip_seg_result;

typedef struct zpaqhip_opts {
  uint32_t struct_size;       /* = sizeof(zpaqhip_opts) */
  uint32_t verify_sha1;       /* 1: check stored SHA-1 of every segment (Decompresser.cs:183-191 contract); hashed on the GPU */
  uint32_t max_concurrent;    /* blocks in flight per launch; 0 = auto (memory-bound) */
  uint32_t kernel;            /* which kernel decodes a block (cross-checks and A/B runs; 0 for production):
                                   0 auto: stored -> zh_store; single CM -> zh_cm, two blocks per workgroup when a launch has
                                     more than 256 of them; min / mid and the models LibZPAQ.makeConfig writes for levels 3 / 4
                                     (`ci1`, `...,1c0,0,511i2`, `ci1,1,1,1,2am`, `...2awm`) -> zh_nibble; max -> zh_chain2;
                                     other models that fit the lane-per-component kernel -> zh_chain (level walk at run time);
                                     the rest -> zh_generic (one lane);
                                   1 every block on zh_generic;
                                   2 / 6 single-CM blocks one / two per workgroup;
                                   3 single-CM blocks on zh_chain;
                                   4 every block that auto sends to zh_nibble, zh_chain2 or zh_store on zh_chain, without model
                                     specialisation (stored blocks included);
                                   5 min / mid / max on zh_chain's forms of the built-in models; the level 3 / 4 models on zh_chain;
                                   9 min / mid on zh_chain2 (bit at a time) instead of zh_nibble; the level 3 / 4 models on zh_chain;
                                   10 as 0, and the E8E9 forms of `lazy2` / `lzpre` in unmodelled blocks (methods x..,5,.. and
                                     x..,6,.. without a model: levels 1 and 2 on executables) stay on zh_store, which runs
                                     their end-of-segment pass wave-wide, instead of being handed to zh_generic in a second
                                     launch.  An opt-in until it becomes the default;
                                   11 as 10, and zh_nibble runs the post-processors `lzpre` and `bwtrle` with E8E9 behind a model
                                     (methods x..,6,..c0,0,511.. and x..,7ci1: levels 3 and 4 on executables, blocks up to
                                     16 MiB) wave-wide — match copies, the inverse BWT and the end-of-segment E8E9 loop —
                                     instead of as translated code on one lane (zpaqhip_stats.e8_wave_segs counts the
                                     segments).  An opt-in;
                                   7 / 8 and any other value: as 0 */
  uint64_t zpaql_budget;      /* runaway-program guard, per run() call: max ZPAQL instructions on the interpreter, max backward
                                 jumps in an ahead-of-time translated program (a translation checks where it can loop);
                                 0 = default (1<<32).  Exceeding it ends the block with ZPAQHIP_E_BUDGET */
  uint64_t batch_blocks;      /* whole-stream forms: blocks per pipeline batch; 0 = default (at least 512 blocks and 32 MiB
                                 of coded bytes per batch, so that every CU has a block) */
  uint64_t queue_blocks;      /* zpaqhip_decompress_multi: blocks per pull from the shared work queue; 0 = default: 256 (one block per
                                 CU of the device that takes the chunk; 512 where every block is a single-CM one), but no more than a
                                 quarter of a device's share of the blocks, so that every device pulls at least four times */
  uint64_t dec_waves;         /* zh_chain with the level walk at run time (kernel 0's "other models", every chain model with kernel 4):
                                 decoder waves (blocks in flight) per compute unit.  0 or 1: one, as before the field existed (it
                                 was reserved[0]).  2 to 4: a launch of more blocks than the device has compute units puts up to
                                 that many waves, one per SIMD, on a unit, as many as the LDS plan of the launch's models allows
                                 (zpaqhip_dec_chain_plan; the smallest of them), and as the blocks, device memory and
                                 max_concurrent call for; above 4 is taken as 4.  The plaintext and the per-segment results never
                                 depend on it; stats.concurrent then counts the blocks in flight (waves with a block).  No effect
                                 on blocks of any other kernel, nor with kernel 3 or 5, nor in the diagnostic build with in-kernel
                                 stamps (ZPAQHIP_PROF set).  The whole-stream forms then make batches of at least 256 x dec_waves
                                 blocks of such models instead of 256.  An opt-in until it becomes the default */
  uint64_t reserved[1];       /* must be 0: the library uses the word for calls of its own */
} zpaqhip_opts;

/* Timing / accounting of the last decode call on a context (the reference's
 * stat() hooks are stubs: Predictor.cs:224-227, Decompresser.cs:196-199). */
typedef struct zpaqhip_stats {
  double kernel_ms;           /* HIP-event time of the decode kernel(s), on the launch stream */
  double init_ms;             /* HIP-event time spent initialising model tables (0 if fused) */
  double h2d_ms, d2h_ms;      /* host<->device copies done by the call (0 for the device form) */
  uint64_t blocks;            /* blocks decoded */
  uint64_t in_bytes;          /* coded bytes consumed */
  uint64_t out_bytes;         /* plaintext bytes produced */
  uint64_t model_bytes;       /* per-block model state (sum over decoded blocks) */
  uint32_t launches;          /* decode kernel launches */
  uint32_t concurrent;        /* blocks in flight per launch (with opts.dec_waves >= 2: the waves with a block of the largest launch) */
  uint32_t kernel_kind;       /* most specialised kernel used: 1 generic, 2 single-CM lanes, 3 lane-per-component */
  uint32_t e8_wave_segs;      /* opts.kernel == 11: segments of modelled blocks whose end-of-segment E8E9 loop ran wave-wide in
                                 the call (a block decoded twice because its plaintext outgrew its staging slot counts
                                 twice); 0 with any other kernel.  Was `reserved` */
} zpaqhip_stats;

typedef struct zpaqhip_ctx zpaqhip_ctx;

/* Reader.read / Writer.write shaped callbacks (Reader.cs:14-25, Writer.cs:19-24). */
typedef int (*zpaqhip_read_fn)(void *user, uint8_t *buf, int n);        /* bytes read, 0 = EOF, <0 = error */
typedef int (*zpaqhip_write_fn)(void *user, const uint8_t *buf, int n); /* 0 = ok, <0 = error */

/* ---- library / context ------------------------------------------------- */
int zpaqhip_version(void);                       /* ZPAQHIP_ABI_VERSION */
const char *zpaqhip_strerror(int status);        /* reference message for a status */
int zpaqhip_device_count(void);                  /* usable HIP devices (0 without a GPU) */
int zpaqhip_ctx_create(int device, zpaqhip_ctx **ctx, zpaqhip_err *err);
void zpaqhip_ctx_destroy(zpaqhip_ctx *ctx);
int zpaqhip_last_stats(const zpaqhip_ctx *ctx, zpaqhip_stats *out);

/* ---- framing: replaces findBlock/findFilename/readComment/readSegmentEnd --
 * (Decompresser.cs:29-108,163-194; Decoder.skip, Decoder.cs:70-98).  Host-side,
 * no GPU needed.  Pass NULL tables with zero capacity to count only; returns
 * ZPAQHIP_E_ARG (with *n_blocks / *n_segs = required) if a table is too small. */
int zpaqhip_scan(const uint8_t *in, size_t in_len,
                 zpaqhip_block *blocks, size_t block_cap, size_t *n_blocks,
                 zpaqhip_segment *segs, size_t seg_cap, size_t *n_segs,
                 zpaqhip_err *err);

/* ---- whole stream, host buffers: replaces LibZPAQ.decompress(Reader, Writer)
 * (LibZPAQ.cs:65-79).  Blocks are decoded concurrently on the context's GPU;
 * plaintext is concatenated in stream order.  *out_len is always the total
 * plaintext size; ZPAQHIP_E_OUTPUT_FULL if it exceeds out_cap. */
int zpaqhip_decompress(zpaqhip_ctx *ctx, const uint8_t *in, size_t in_len,
                       uint8_t *out, size_t out_cap, size_t *out_len,
                       const zpaqhip_opts *opts, zpaqhip_err *err);

/* ---- same, but per-segment outcomes are handed back instead of aborting at the first bad
 * block: this is what a step-wise Decompresser mirror (findBlock / findFilename /
 * decompress(n) / readSegmentEnd, Decompresser.cs:29-194) needs to raise an error only when
 * the caller reaches the failing segment, as the reference does.  results[i] describes
 * segment i of zpaqhip_scan's table (out_off relative to `out`).  Returns
 * ZPAQHIP_E_ARG with *n_results = required count if result_cap is too small. */
int zpaqhip_decompress_segments(zpaqhip_ctx *ctx, const uint8_t *in, size_t in_len,
                                uint8_t *out, size_t out_cap, size_t *out_len,
                                zpaqhip_seg_result *results, size_t result_cap, size_t *n_results,
                                const zpaqhip_opts *opts, zpaqhip_err *err);

/* ---- same, streaming through Reader/Writer-shaped callbacks -------------- */
int zpaqhip_decompress_cb(zpaqhip_ctx *ctx, zpaqhip_read_fn read_fn, zpaqhip_write_fn write_fn,
                          void *user, const zpaqhip_opts *opts, zpaqhip_err *err);

/* ---- whole stream on several GPUs of one node (BASELINE.json configs[3]) ----
 * LibZPAQ.decompress(Reader, Writer) (LibZPAQ.cs:65-79) for a caller that owns more than one GPU and no
 * torch.distributed ranks (the C# host): one context and one host thread per entry of `devices` (a device may be
 * listed more than once; the contexts then share its memory budget).  The threads pull chunks of
 * opts->queue_blocks blocks from ONE work queue ordered by estimated cost (zpaqhip_block_costs), so a device that is
 * faster takes more chunks; plaintext arrives in `out` in stream order.  With a decimal size in every segment comment
 * (LibZPAQ.compressBlock writes it, LibZPAQ.cs:298-300) every device copies its blocks straight to their final place;
 * a block without a plausible size, or with a wrong one, is kept in a host buffer and put in place (it and what
 * follows it) when all sizes are known — no block is decoded twice.  A damaged block ends the call with its error
 * after every block before it has been delivered (*out_len = their bytes).  (Difference to zpaqhip_decompress /
 * zpaqhip_decompress_cb, which write as they decode like the reference: those also deliver the bytes the damaged block
 * itself produced before its error; this entry point places whole blocks only, so its plaintext is a prefix of theirs.
 * Pinned by test_multi_device_entry_point_with_contexts_sharing_this_gpu.)  No context is needed; the ones the call
 * makes are kept for the next call (zpaqhip_multi_trim); idle ones beyond what a call uses on a device, and all idle
 * ones of a device whose memory a later launch needs, are released by the library itself.
 * The _stats form also fills per_device[0..n_devices) (kernel_ms, blocks, ... summed over the chunks a device took;
 * launches = chunks). */
int zpaqhip_decompress_multi(const int *devices, size_t n_devices, const uint8_t *in, size_t in_len,
                             uint8_t *out, size_t out_cap, size_t *out_len,
                             const zpaqhip_opts *opts, zpaqhip_err *err);
int zpaqhip_decompress_multi_stats(const int *devices, size_t n_devices, const uint8_t *in, size_t in_len,
                                   uint8_t *out, size_t out_cap, size_t *out_len,
                                   const zpaqhip_opts *opts, zpaqhip_stats *per_device, zpaqhip_err *err);

/* zpaqhip_decompress_multi keeps the contexts it has used (one per device thread: tables, arena, streams) for its next
 * call; this destroys the idle ones and gives their device memory back. */
void zpaqhip_multi_trim(void);

/* Estimated decode cost of each block of a scanned stream, the weight every multi-GPU plan here uses: plaintext bytes
 * (the comment's decimal size when plausible, else 4 x coded bytes) x the cycles per plaintext byte of the kernel
 * the block's header selects (measured).  Decode time of a block is its bit count times the depth of its model
 * (Predictor.cs:245-475 runs once per bit), not its coded size.  Host-side, no GPU needed. */
int zpaqhip_block_costs(const uint8_t *in, size_t in_len, const zpaqhip_block *blocks, size_t n_blocks,
                        const zpaqhip_segment *segs, size_t n_segs, uint64_t *cost, zpaqhip_err *err);

/* ---- explicit block-table form, device-resident buffers ------------------
 * Replaces the per-block inner loop Decompresser.decompress(-1)
 * (Decompresser.cs:121-153) for a set of blocks.  `d_in` is the whole stream in
 * device memory; it must be 4-byte aligned and readable up to in_len rounded up to
 * a multiple of 4 (the kernels fetch the coded bytes as aligned dwords); `ids[0..n_ids)` selects the blocks this GPU decodes (NULL =
 * all, in table order) — the multi-GPU scheduler gives each rank its shard.
 * Block ids[i] writes its plaintext (all segments, concatenated) at
 * d_out + out_off[i], at most out_cap[i] bytes; bytes past the capacity are
 * counted, not written (status ZPAQHIP_E_OUTPUT_FULL).  results[] has one entry
 * per segment of the table (entries of blocks not in ids are left untouched);
 * out_off in a result is relative to d_out.  `hip_stream` is a hipStream_t (NULL
 * = the context's own stream); the call returns after the stream work has
 * completed.  `h_in` is an optional host copy of the same stream; when NULL the
 * few header bytes the host needs are fetched from d_in. */
int zpaqhip_decode_blocks_device(zpaqhip_ctx *ctx, const void *d_in, const uint8_t *h_in, size_t in_len,
                                 const zpaqhip_block *blocks, size_t n_blocks,
                                 const zpaqhip_segment *segs, size_t n_segs,
                                 const uint32_t *ids, size_t n_ids,
                                 void *d_out, const uint64_t *out_off, const uint64_t *out_cap,
                                 zpaqhip_seg_result *results,
                                 const zpaqhip_opts *opts, void *hip_stream, zpaqhip_err *err);

/* ---- framing of a device-resident stream: zpaqhip_scan with the stream in device memory ------------------------------------
 * `d_in` is the whole stream on the context's device, under the requirements of zpaqhip_decode_blocks_device: 4-byte aligned
 * (ZPAQHIP_E_ARG otherwise) and readable up to in_len rounded up to a multiple of 4; nothing behind that is touched.  The
 * contract is zpaqhip_scan's, field for field, on the same bytes: the same tables (host memory), model_mem included, the same
 * return code and err.code / block / segment / msg, the same prefix of blocks and segments kept in front of framing damage,
 * count-only with NULL tables of zero capacity, ZPAQHIP_E_ARG with the required counts when a table is too small.  The
 * stream stays where it is: one streaming kernel (zh_scan.hip) lists where findBlock's hash matches and where runs of four
 * or more zero bytes lie, every listed tag is parsed in parallel, and one short serial pass on the device picks the blocks
 * (DESIGN.md 2.9).  Only the sums of the lists, the scan's result record and the tables cross the bus.  `hip_stream` is a
 * hipStream_t (NULL = the context's own stream) on which d_in is read; the call returns after its work has completed.
 * zpaqhip_last_stats: kernel_ms = init_ms = the scan's kernels, launches = their number, blocks, in_bytes = in_len. */
int zpaqhip_scan_device(zpaqhip_ctx *ctx, const void *d_in, size_t in_len,
                        zpaqhip_block *blocks, size_t block_cap, size_t *n_blocks,
                        zpaqhip_segment *segs, size_t seg_cap, size_t *n_segs,
                        void *hip_stream, zpaqhip_err *err);

/* ---- whole stream, device buffers: LibZPAQ.decompress(Reader, Writer) (LibZPAQ.cs:65-79) with both ends in device memory ---
 * d_in as for zpaqhip_scan_device, whose tables the call works from; the plaintext arrives in stream order at d_out.
 * *out_len is always the total; when it exceeds out_cap the call returns ZPAQHIP_E_OUTPUT_FULL and nothing is written at or
 * past d_out + out_cap.  opts (kernel, verify_sha1, dec_waves, max_concurrent, zpaql_budget) mean what they mean for
 * zpaqhip_decompress; the SHA-1 is computed on the device.  results (optional: NULL with result_cap 0) receives one record
 * per segment as zpaqhip_decompress_segments does, out_off relative to d_out; *n_results (optional) their number;
 * ZPAQHIP_E_ARG with *n_results = the required count when result_cap is too small.
 * Placement: as long as every block so far has a plausible decimal size in its comments, a block is decoded straight to its
 * final place.  The first block without one, and what follows it, is decoded to staging slots (those of zpaqhip_decompress)
 * and gathered into place by the packing kernel (zh_frame.hip) in one launch.  A size that turns out wrong (too small: the
 * block reports its real length; too large: a gap) makes that block and what follows it move.  No block is decoded more than
 * twice.  No plaintext and no coded byte crosses the bus: the tables, the block headers and the per-segment results do.
 * A damaged block: zpaqhip_decompress_multi's contract, not zpaqhip_decompress's: whole blocks only; every block in front of
 * the damaged one is delivered, *out_len = their bytes, and the damaged block's error is returned (the bytes that block
 * produced before its error are not delivered).  A framing error behind the last good block is returned after those blocks
 * have been delivered, as by zpaqhip_decompress.
 * zpaqhip_last_stats: h2d_ms = d2h_ms = 0; init_ms = the scan's kernels, which also count in kernel_ms and launches (as do
 * the packing kernel's); blocks, in_bytes, model_bytes, concurrent, kernel_kind as for zpaqhip_decompress. */
int zpaqhip_decompress_device(zpaqhip_ctx *ctx, const void *d_in, size_t in_len,
                              void *d_out, size_t out_cap, size_t *out_len,
                              zpaqhip_seg_result *results, size_t result_cap, size_t *n_results,
                              const zpaqhip_opts *opts, void *hip_stream, zpaqhip_err *err);

/* zh_chain's LDS plan for the model of a block header (`hdr` as the stream carries it: hsize lo, hsize hi, hh hm ph pm n,
 * components, 0, HCOMP, 0): *waves = the most decoder waves one compute unit holds for it, 1 to 4 (what opts.dec_waves uses
 * at most), or 0 for a model that kernel does not take; *lds_bytes = the LDS of a workgroup of that many waves (the shared
 * tables and, per wave, the model's ICM / ISSE tables and a fixed part), at most 163 840, or 0.  Host-side, no GPU needed. */
int zpaqhip_dec_chain_plan(const uint8_t *hdr, size_t hdr_len, uint32_t *waves, uint32_t *lds_bytes, zpaqhip_err *err);

/* Device-side copies of the model-independent tables, for parity tests
 * (Predictor.cs:48-79 squash/stretch/dt/dt2k, StateTable.cs:21-149).
 * squash 4096 u16, stretch 32768 i16, dt 1024 i32, dt2k 256 i32, ns 1024 u8;
 * any pointer may be NULL.  The values are read back FROM THE DEVICE. */
int zpaqhip_read_device_tables(zpaqhip_ctx *ctx, uint16_t *squash, int16_t *stretch,
                               int32_t *dt, int32_t *dt2k, uint8_t *ns, zpaqhip_err *err);

/* Decompresser.pcomp(Writer) (Decompresser.cs:155-158, ZPAQL.write(out, true) ZPAQL.cs:158-179): the PCOMP
 * program of block `block` (index into zpaqhip_scan's table) as the reference writes it: length low byte, length
 * high byte, program bytes.  *out_len = 0 and ZPAQHIP_OK when the block has no PCOMP (pcomp() returns false).
 * ZPAQHIP_E_OUTPUT_FULL with *out_len = bytes needed when out_cap is too small.  The program is part of the coded
 * data: this call decodes the first bytes of the block (up to the end of the post-processor header) on the GPU. */
int zpaqhip_block_pcomp(zpaqhip_ctx *ctx, const uint8_t *in, size_t in_len, uint32_t block,
                        uint8_t *out, size_t out_cap, size_t *out_len, zpaqhip_err *err);

/* ---- compression: the other half of the reference's public surface ----------------------------------------------
 * LibZPAQ.compress / Compressor / Encoder (Compressor.cs:27-299, Encoder.cs:26-104) at the Compressor level: the caller
 * gives the model (header and optional PCOMP); zpaqhip_compress_method_blocks below takes a method's numbers instead.
 * Every coded byte comes out of a HIP kernel. */
typedef struct zpaqhip_compress_opts {
  uint32_t struct_size;     /* = sizeof(zpaqhip_compress_opts) */
  uint32_t flags;           /* bit0: store SHA-1 (253 + digest, else 254); bit1: write the 13-byte tag; bit2 (zpaqhip_compress_method_blocks
                               only): accept level 3 (BWT) methods; bit3 (zpaqhip_compress_method_blocks only): a level 1 / 2 method
                               with args[5] - args[0] >= 21 is parsed by the reference's suffix-array search (see
                               zpaqhip_lzsa_blocks); no effect on any other method; bit4 (zpaqhip_compress_method_blocks only): a
                               level 1 / 2 method with args[5] - args[0] < 21 is parsed by the reference's hash-table search
                               (see zpaqhip_lzht_blocks); no effect on any other method; bits 3 and 4 may be given together;
                               bit5 (value 32, every compressing call): verify (Compressor.setVerify, Compressor.cs:118-121): each
                               batch's coded sequences run through the block's own post-processor on the device before the
                               encoders see them, and a block that does not come back as its plaintext fails the call (see
                               zpaqhip_verify_blocks); NULL opts = 3 */
  uint32_t kernel;          /* 0 auto: single-CM models of the `a<<= K  *d=a  halt` shape (K >= 9) on the window-parallel
                               encoder, the rest on the generic one; 1 every block on the generic encoder (cross-check);
                               2 as 0, but models that fit the lane-per-component kernel (ICM / ISSE / MATCH / MIX chains of at
                               most 64 components and 4 mixers: min, mid, max, the models of the method strings) on the
                               lane-per-component encoder (zh_enc_chain.hip); an opt-in until it becomes the default */
  uint32_t enc_waves;       /* lane-per-component encoder: encoder waves (blocks in flight) per compute unit.  0 automatic: a
                               launch of more blocks than the device has compute units puts up to four waves, one per SIMD,
                               on a unit, as many as the model's LDS plan allows (zpaqhip_enc_chain_plan) and the blocks
                               and device memory call for; 1 one wave per unit; 2 to 4 a cap on the automatic choice; above
                               4 ZPAQHIP_E_ARG.  The coded bytes never depend on it.  No effect unless kernel == 2 routes a
                               block to that encoder */
  uint64_t batch_blocks;    /* blocks per device batch; 0 = sized from free device memory */
  uint64_t slot_bytes;      /* test knob: device bytes reserved per block for coded data before the overflow path; 0 = auto
                               (coded bytes + 1/8 + 4096).  A block that does not fit is coded again with a worst-case slot:
                               the output never changes */
  uint64_t reserved[2];
} zpaqhip_compress_opts;

/* Compressor.startBlock(hcomp) + startSegment(filename, size) + postProcess(pcomp) + compress() + endSegment(sha1) +
 * endBlock() for each of n_blocks blocks (LibZPAQ.cs:296-323 framing, one segment per block).  `hdr` is the block header
 * as the stream carries it (hsize lo, hsize hi, hh hm ph pm n, components, 0, HCOMP, 0); `pcomp` the PCOMP program as
 * Compressor.postProcess sends it (NULL / 0 = PASS).  Block i codes in[in_off[i], in_off[i+1]); its size comment and
 * SHA-1 describe orig[orig_off[i], orig_off[i+1]) (NULL = the coded bytes); filenames[i] (NULL, or a NULL entry = empty)
 * is its segment's name.  out receives the blocks in order; block_off[0..n_blocks] (optional) their offsets.
 * ZPAQHIP_E_OUTPUT_FULL with *out_len = the exact size needed when out_cap is short.  Modelled headers only (n >= 1):
 * n == 0 gives ZPAQHIP_E_ARG.  zpaqhip_last_stats: kernel_ms = both encoder passes (and any re-encoding of overflowed
 * blocks), init_ms = the model pass of the window-parallel CM encoder alone (part of kernel_ms; the rest is its coder pass
 * and the generic encoder), launches = encoder launches (one more per batch with an overflowed block), in_bytes =
 * plaintext, out_bytes = the stream, kernel_kind = 3 when a block ran on the lane-per-component encoder (opts.kernel
 * == 2; its time is part of kernel_ms, an overflowed block of it is coded again on the same encoder), 2 when one ran on
 * the window-parallel CM encoder, else 1; concurrent = the blocks in flight (encoder waves with a block) of the call's
 * largest launch of the lane-per-component encoder, 0 when no block ran there. */
int zpaqhip_compress_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                            const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                            const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                            uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                            const zpaqhip_compress_opts *opts, zpaqhip_err *err);

/* The lane-per-component encoder's LDS plan for the model of a block header (`hdr` as for zpaqhip_compress_blocks):
 * *waves = the most encoder waves one compute unit holds for it, 1 to 4 (what opts.enc_waves == 0 uses at most), or 0 for
 * a model that encoder does not take; *lds_bytes = the LDS of a workgroup of that many waves (the shared tables and, per
 * wave, the model's ICM / ISSE tables and a fixed part), at most 163 840, or 0.  Host-side, no GPU needed. */
int zpaqhip_enc_chain_plan(const uint8_t *hdr, size_t hdr_len, uint32_t *waves, uint32_t *lds_bytes, zpaqhip_err *err);

/* ---- compression with a method: LibZPAQ.compressBlock (LibZPAQ.cs:296-323) with the pre-processing of LZBuffer and E8E9 ----
 * args are the nine numbers of an expanded method string as LibZPAQ.makeConfig reads them (LibZPAQ.cs:394-416; what
 * zpaqsharp_amd.method.parse_args returns).  level = args[1] & 3; 4 <= args[1] <= 7 applies forward E8E9 (LibZPAQ.cs:372-384)
 * first.  Level 1 writes LZBuffer's bit-packed codes, level 2 its byte-aligned ones (LZBuffer.cs:96-112), with a greedy
 * parse: key k = max(4, args[2]) (level 1) or max(args[2], 3) (level 2); position i starts a match iff the nearest earlier
 * position with the same k bytes lies within 2^23 - 1 (level 1) or 2^24 - 1 (level 2); the match takes as many bytes as
 * match, up to 2^16 (level 1) or args[2] + 319 (level 2).  Level 3 writes LZBuffer's Burrows-Wheeler transform
 * (LZBuffer.cs:228-240: n + 5 bytes for n, the end of the block sorting below every byte) from a suffix array built by
 * prefix doubling (zh_pre_bwt.hip); it is an opt-in: zpaqhip_compress_method_blocks takes it with bit2 of opts.flags,
 * zpaqhip_bwt_blocks always.  Everything runs on the GPU (zh_pre_lz.hip, zh_pre_bwt.hip).
 * A second opt-in (bit3 of opts.flags, zpaqhip_lzsa_blocks always) replaces the greedy parse of a level 1 / 2 method with
 * args[5] - args[0] >= 21 by the one LZBuffer itself makes for such a method (LZBuffer.cs:246-283, :329-383): a search of up
 * to 2^args[4] - 1 neighbours on each side in suffix order, scored 8 * length - lg(offset) - 11, with args[6] bytes of
 * look-ahead, matches up to 49 152 bytes and a literal flush every 4096; the bytes are LZBuffer's (zh_pre_lzsa.hip).  That
 * route refuses, with ZPAQHIP_E_ARG, level 1 with args[2] < 4, args[2] or args[6] above 255, args[4] above 30 and a block
 * longer than 2^24 bytes (offsets of 2^24 and more are not written).
 * A third opt-in (bit4 of opts.flags, zpaqhip_lzht_blocks always) does the same for a level 1 / 2 method with
 * args[5] - args[0] < 21: LZBuffer's hash-table search (LZBuffer.cs:285-327, :349-368) of the 2^args[4] slots around the
 * hash of the next args[2] bytes in a table of 2^args[5] entries with 12 - args[0] check bits, scored
 * 8 * length - lg(offset) - 2 * (literals pending) - 11, matches up to 49 152 bytes, a literal flush every 4096; level 2
 * with args[2] > 64 searches nothing (zh_pre_lzht.hip).  That route refuses, with ZPAQHIP_E_ARG: args[3] != 0 (the second
 * hash order) and args[6] != 0 (look-ahead), level 1 with args[2] < 4, level 2 with args[2] < 2, args[2] > 255,
 * args[0] > 11, args[4] > args[5] or args[4] > 6, args[5] > 30 and a block longer than 2^24 bytes.
 * Refused with ZPAQHIP_E_ARG: level 3 (BWT) without the opt-in (zpaqhip_preprocess_blocks: always); level 2 with args[2]
 * outside 1..64; at level 1 or 2 a block longer than 2^(args[0] + 20) bytes (its offsets would wrap the PCOMP's M), at
 * level 3 than 2^(args[0] + 20) - 4096 bytes (LibZPAQ.cs:289), or than 2^31 - 1 bytes. */

/* The pre-processed bytes of each block in[in_off[i], in_off[i+1]), back to back in out; out_off[0..n_blocks] (optional)
 * their offsets.  ZPAQHIP_E_OUTPUT_FULL with *out_len = the exact size needed when out_cap is short.
 * zpaqhip_last_stats: kernel_ms = init_ms = the pre-processing kernels. */
int zpaqhip_preprocess_blocks(zpaqhip_ctx *ctx, const int32_t args[9], const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                              uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err);

/* LZBuffer's level 3 (BWT) of each block in[in_off[i], in_off[i+1]), after forward E8E9 when doe8 is not 0: n + 5 bytes per
 * block, back to back in out; out_off, capacity and statistics as for zpaqhip_preprocess_blocks.  The only size limit is
 * 2^31 - 1 bytes per block. */
int zpaqhip_bwt_blocks(zpaqhip_ctx *ctx, int doe8, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                       uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err);

/* LZBuffer's codes of each block for a level 1 / 2 method with args[5] - args[0] >= 21 (ZPAQHIP_E_ARG for any other), from
 * its suffix-array search, after forward E8E9 when 4 <= args[1] <= 7; out_off, capacity and statistics as for
 * zpaqhip_preprocess_blocks (init_ms covers the suffix sort, launches counts its kernels as zpaqhip_bwt_blocks does). */
int zpaqhip_lzsa_blocks(zpaqhip_ctx *ctx, const int32_t args[9], const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                        uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err);

/* LZBuffer's codes of each block for a level 1 / 2 method with args[5] - args[0] < 21 (ZPAQHIP_E_ARG for any other, and for
 * what the route refuses, see above), from its hash-table search, after forward E8E9 when 4 <= args[1] <= 7; out_off,
 * capacity and statistics as for zpaqhip_lzsa_blocks (init_ms covers the sort of the positions by hash slot). */
int zpaqhip_lzht_blocks(zpaqhip_ctx *ctx, const int32_t args[9], const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                        uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err);

/* compressBlock of a method for each block, one segment per block, framing as zpaqhip_compress_blocks.  hdr / pcomp are
 * the block header and PCOMP of makeConfig's text for the method; the size comment and SHA-1 (zh_sha1_dev) describe the
 * plaintext.  n >= 1 headers: the pre-processed bytes stay in device memory and go to the encoders of
 * zpaqhip_compress_blocks, whose opts (kernel, batch_blocks, slot_bytes) apply.  n == 0 headers: the store layout of
 * Encoder.compress without a model (selector or PCOMP header, then the bytes, in 4-byte big-endian length-prefixed chunks
 * of 65 536 bytes, then four zero bytes) in a level 2 block (Compressor.cs:92-96); opts.batch_blocks applies.
 * zpaqhip_last_stats: init_ms = the pre-processing alone, kernel_ms = pre-processing and encoder passes, kernel_kind as
 * for zpaqhip_compress_blocks for modelled blocks (3 with opts.kernel == 2 for the chain models of levels 3 and 4) and 0
 * when every block is unmodelled. */
int zpaqhip_compress_method_blocks(zpaqhip_ctx *ctx, const int32_t args[9], const uint8_t *hdr, size_t hdr_len,
                                   const uint8_t *pcomp, size_t pcomp_len, const uint8_t *in, const uint64_t *in_off,
                                   size_t n_blocks, const char *const *filenames, uint8_t *out, size_t out_cap, size_t *out_len,
                                   uint64_t *block_off, const zpaqhip_compress_opts *opts, zpaqhip_err *err);

/* ---- compression of device-resident blocks: the two calls above with the plaintext and the stream in device memory --------
 * zpaqhip_compress_blocks_device is zpaqhip_compress_blocks, zpaqhip_compress_method_blocks_device is
 * zpaqhip_compress_method_blocks (same flags, bits 0 to 4 of opts.flags), with `d_in`, `d_orig` (optional) and `d_out` device
 * pointers on the context's device; in_off, orig_off, filenames, block_off, out_len, hdr and pcomp stay host memory.
 * `hip_stream` is a hipStream_t (NULL = the context's own stream) on which every read of d_in / d_orig and every write of
 * d_out is ordered; the call returns after the stream's work has completed.  The contract is the host forms': d_out[0,
 * *out_len) holds exactly the bytes the host form writes for the same arguments, block_off and zpaqhip_last_stats are the
 * same (launches also counts the packing kernel, zh_frame.hip: its launch that frames a batch, whose time is part of
 * kernel_ms, and, without pre-processing, the one that stages a batch in place of the host form's upload, which like that
 * upload is not timed), and with out_cap too small the call
 * returns ZPAQHIP_E_OUTPUT_FULL with *out_len = the bytes needed, every block that fits in whole written and nothing written
 * at or past d_out + out_cap.  No plaintext and no coded byte crosses the bus: per batch the results of the encoders, the
 * digests (20 bytes per block) and the frame table (where each block's head, body and tail go) do.
 * Alignment: none is asked of d_out, d_in or d_orig.  Heads and tails are built on the host; the packing kernel gathers
 * head || body || tail of every block into d_out.  The encoders and the pre-processing work on an aligned device copy of a
 * batch's input (device to device), as they do on the staged copy of the host forms; SHA-1 reads d_orig, when given, where
 * it is.  Device memory is read in aligned 16-byte groups that hold at least one byte of a block, as any allocation of
 * hipMalloc allows. */
int zpaqhip_compress_blocks_device(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                   const void *d_in, const uint64_t *in_off, size_t n_blocks,
                                   const void *d_orig, const uint64_t *orig_off, const char *const *filenames,
                                   void *d_out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                                   const zpaqhip_compress_opts *opts, void *hip_stream, zpaqhip_err *err);
int zpaqhip_compress_method_blocks_device(zpaqhip_ctx *ctx, const int32_t args[9], const uint8_t *hdr, size_t hdr_len,
                                          const uint8_t *pcomp, size_t pcomp_len, const void *d_in, const uint64_t *in_off,
                                          size_t n_blocks, const char *const *filenames, void *d_out, size_t out_cap,
                                          size_t *out_len, uint64_t *block_off, const zpaqhip_compress_opts *opts,
                                          void *hip_stream, zpaqhip_err *err);

/* ---- solid blocks: several segments per block (Compressor.startSegment .. endSegment, repeated; Compressor.cs:133-248) ------
 * zpaqhip_compress_blocks[_device] with one more table: block i holds the segments [seg_first[i], seg_first[i + 1]) of the
 * call, at least one (seg_first[0] == 0; n_segs = seg_first[n_blocks], below 2^32).  in_off, orig_off (with `orig`) and
 * filenames are then PER SEGMENT: n_segs + 1 offsets, n_segs names; segment s codes in[in_off[s], in_off[s + 1]), its size
 * comment and SHA-1 describe orig[orig_off[s], orig_off[s + 1]) (NULL = the coded bytes).  block_off[0..n_blocks] stays per
 * block.  A block is what Compressor writes for
 *   startBlock(hdr); for each segment: startSegment(filename, size), postProcess(pcomp) (it acts in the first segment only,
 *   Compressor.cs:158), compress(its bytes), endSegment(sha1 or none); endBlock()
 * behind the tag (bit1 of opts.flags): the model, the coder's interval and the post-processor's state carry over from a
 * segment to the next, which is what packing many small files into one block is for.  The caller sees to it that the
 * segments' coded bytes are what the post-processor turns into their described bytes one after the other.
 * opts: bits 0 and 1 of flags, kernel, enc_waves, batch_blocks and slot_bytes with the meaning they have for
 * zpaqhip_compress_blocks; any other bit of flags (the method opt-ins, verify) gives ZPAQHIP_E_ARG.  A block of one segment
 * takes the encoder it takes there and comes out byte for byte the same.  A block of several segments never takes the
 * window-parallel CM encoder: with kernel == 2 a single-CM model's goes to the lane-per-component encoder, else to the
 * generic one.  ZPAQHIP_E_ARG, before the device is touched, also for a block without a segment, seg_first or offsets that
 * decrease (err.block tells the block, err.segment the segment within it) and an n == 0 header.  zpaqhip_last_stats,
 * ZPAQHIP_E_OUTPUT_FULL (whole blocks only) and the device form's contract (pointers, stream, alignment, nothing at or past
 * d_out + out_cap, no plaintext or coded byte over the bus; per segment a digest, an end offset and a table entry
 * cross it) are those of zpaqhip_compress_blocks and zpaqhip_compress_blocks_device. */
int zpaqhip_compress_solid_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                  const uint8_t *in, const uint64_t *in_off, const uint64_t *seg_first, size_t n_blocks,
                                  const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                                  uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                                  const zpaqhip_compress_opts *opts, zpaqhip_err *err);
int zpaqhip_compress_solid_blocks_device(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp,
                                         size_t pcomp_len, const void *d_in, const uint64_t *in_off, const uint64_t *seg_first,
                                         size_t n_blocks, const void *d_orig, const uint64_t *orig_off,
                                         const char *const *filenames, void *d_out, size_t out_cap, size_t *out_len,
                                         uint64_t *block_off, const zpaqhip_compress_opts *opts, void *hip_stream,
                                         zpaqhip_err *err);

/* ---- a method per block: what LibZPAQ.compressBlock does with a numeric level (LibZPAQ.cs:84-283), device-resident ----------
 * zpaqhip_compress_method_blocks_device for blocks that do not all take the same method: methods[0, n_methods) is the list
 * (args, hdr and pcomp of each as for zpaqhip_compress_method_blocks; `reserved` must be 0), method_of[i] the entry block i
 * takes.  d_out[0, *out_len) holds the blocks in input order, block i exactly the bytes zpaqhip_compress_method_blocks writes
 * for it with methods[method_of[i]] and the same opts (bits 0 to 4 of opts.flags apply to every method), block_off[0..n_blocks]
 * their offsets.  With out_cap too small: ZPAQHIP_E_OUTPUT_FULL with *out_len = the bytes needed, every block that fits in
 * whole written (the offsets only grow, so these are the first blocks of the call) and nothing written at or past d_out +
 * out_cap.  ZPAQHIP_E_ARG before the device is touched: a NULL context, d_out == NULL with a capacity, decreasing offsets,
 * n_methods == 0 with blocks, a method_of[i] >= n_methods (err->block = i), a non-zero `reserved`, and whatever the method form
 * refuses for a method and the length of a block that takes it; err->block is always the block's index in this call.  A
 * method that no block takes is not checked against any block.
 * How: the blocks of each method that is used run as one group through the method form's path, whose stream goes to a scratch
 * stream in device memory that the call owns; the groups lie back to back in it.  The scratch grows to what the groups
 * turn out to need (it doubles, keeping what it holds; ZPAQHIP_E_DEVICE_MEM when it cannot), so it ends between one and two
 * times the size of the output.  One more launch of the packing kernel then gathers the blocks into d_out in input order:
 * one device-to-device pass over the coded bytes.  No plaintext and no coded byte crosses the bus.  Alignment and hip_stream
 * as for the two calls above.
 * zpaqhip_last_stats: kernel_ms and init_ms summed over the groups, the gather's time added to kernel_ms; launches = the
 * groups' launches plus the gather's; blocks, in_bytes and out_bytes of the whole call; kernel_kind and concurrent the
 * largest among the groups; and, for this call only, model_bytes = the scratch stream's capacity at the end of the call and
 * e8_wave_segs = the gather launch's own time in microseconds (both 0 in every other compressing call). */
typedef struct zpaqhip_method {          /* one entry of the method list of a mixed call */
  int32_t args[9];                       /* as for zpaqhip_compress_method_blocks */
  uint32_t reserved;                     /* must be 0 */
  const uint8_t *hdr;   size_t hdr_len;
  const uint8_t *pcomp; size_t pcomp_len;
} zpaqhip_method;

int zpaqhip_compress_mixed_blocks_device(zpaqhip_ctx *ctx, const zpaqhip_method *methods, size_t n_methods,
                                         const uint32_t *method_of, const void *d_in, const uint64_t *in_off, size_t n_blocks,
                                         const char *const *filenames, void *d_out, size_t out_cap, size_t *out_len,
                                         uint64_t *block_off, const zpaqhip_compress_opts *opts, void *hip_stream,
                                         zpaqhip_err *err);

/* ---- the pre/post-processor test (Compressor.setVerify, Compressor.cs:118-121; endSegmentChecksum, :251-281) --------------
 * zpaqhip_verify_blocks is endSegmentChecksum(&size) for a set of blocks: block i's pre-processed bytes in[in_off[i],
 * in_off[i+1]) are post-processed on the GPU exactly as PostProcessor.write would after the decoder (the selector for
 * `pcomp`, the program fed byte by byte, run(-1) at the end of the segment, with H and M of the sizes `hdr` gives: only ph
 * and pm of the header matter), and results[i] tells how many bytes came out, their SHA-1 and, with `orig`, the offset of
 * the first byte that differs from orig[orig_off[i], orig_off[i+1]) (the shorter length when one is a prefix of the other).
 * status is ZPAQHIP_OK, ZPAQHIP_E_VERIFY when the plaintext is given and differs, or the post-processor's own error
 * (ZPAQHIP_E_ZPAQL, ZPAQHIP_E_PP_*, ZPAQHIP_E_BUDGET); out_len and sha1 then describe what it wrote before it stopped.
 * `pcomp` NULL / 0 = PASS: size and SHA-1 of the bytes themselves.  The reference's programs (lazy2, lzpre, bwtrle; the
 * first two with E8E9 too) run on the wave-wide post-processors of the decoder (zh_store.hip), one workgroup per block;
 * every other program on its translation or on the ZPAQL VM, one lane per block.  The post-processed bytes stay in device
 * memory that the call owns; only the records cross the bus (and, in the host form, the arguments).  The call returns
 * ZPAQHIP_OK when it ran, whatever the records say.  zpaqhip_last_stats: kernel_ms = the pass (post-processors, SHA-1,
 * compare), launches = its launches, blocks, in_bytes = pre-processed bytes, out_bytes = bytes post-processed.
 *
 * The compressing calls run the same pass with bit5 of zpaqhip_compress_opts.flags, in the batch loop between pre-processing
 * and the encoders (zpaqhip_compress_blocks[_device]: over `in` as given, against `orig`, or against `in` itself without
 * one).  A failing block ends the call with its record's status and err->block = the lowest failing index of that batch
 * (zpaqhip_compress_mixed_blocks_device: of the first group that fails, in the order the call takes the groups), *out_len = 0
 * and the contents of out unspecified: a verified call delivers all blocks or none.  With every block passing the stream
 * is byte for byte the one without the bit; kernel_ms and launches also count the pass. */
typedef struct zpaqhip_verify_result {
  int32_t status;        /* ZPAQHIP_OK, ZPAQHIP_E_VERIFY, or the post-processor's own error */
  uint32_t reserved;
  uint64_t out_len;      /* bytes the post-processor wrote */
  uint64_t first_diff;   /* UINT64_MAX: equal, or no plaintext given */
  uint8_t sha1[20];      /* of those bytes */
  uint32_t reserved2;
} zpaqhip_verify_result; /* 48 bytes */

int zpaqhip_verify_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                          const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                          const uint8_t *orig, const uint64_t *orig_off, zpaqhip_verify_result *results, zpaqhip_err *err);

/* The same with `d_in` and `d_orig` (optional) in device memory on the context's device; the offsets and the records stay
 * host memory.  No alignment is asked of either; both are read where they lie.  `hip_stream` as for
 * zpaqhip_compress_blocks_device. */
int zpaqhip_verify_blocks_device(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                 const void *d_in, const uint64_t *in_off, size_t n_blocks,
                                 const void *d_orig, const uint64_t *orig_off, zpaqhip_verify_result *results,
                                 void *hip_stream, zpaqhip_err *err);

/* ---- the data analysis of LibZPAQ.compressBlock's numeric levels 5..9 (LibZPAQ.cs:242-255) -------------------------------
 * The histogram of repetition gaps of each block p = in[in_off[i], in_off[i+1]): with pt[256] and r[4096] all zero,
 *     for j in 0..n-1:  k = j - pt[p[j]];  if 0 < k < 4096: ++r[k];  pt[p[j]] = j
 * and hist[i * 4096 + k] = r[k] (hist[i * 4096] = 0).  As in the reference pt starts at 0, so a byte value first seen at
 * position j counts as gap j when 0 < j < 4096, and position 0 counts nothing.  compressBlock picks the periodic context
 * models of a level 5..9 method from r (zpaqsharp_amd.method.expand_level does the same from this histogram).  Computed on
 * the GPU (zh_analyze.hip), in batches sized like those of zpaqhip_preprocess_blocks.  A block holds at most 2^31 - 1
 * bytes (ZPAQHIP_E_ARG beyond); an empty block gives zeros.  zpaqhip_last_stats: kernel_ms = init_ms = the kernel,
 * launches = its launches, h2d_ms / d2h_ms = the host's time in the copy of the plaintext in and of the histograms out,
 * in_bytes = plaintext, out_bytes = n_blocks * 16 384. */
int zpaqhip_gap_hist_blocks(zpaqhip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, uint32_t *hist,
                            zpaqhip_err *err);

/* zpaqhip_gap_hist_blocks with the plaintext in device memory: block i is d_in[in_off[i], in_off[i+1]) on the context's
 * device; in_off and hist stay host memory, and the histograms (16 384 bytes per block) are all that crosses the bus.  The
 * same limits and the same histograms.  `hip_stream` as for zpaqhip_compress_blocks_device.  Alignment: none is asked of
 * d_in; the kernel reads it where it is, in aligned 16-byte groups that hold at least one byte of the block it walks.
 * zpaqhip_last_stats as for the host form, with h2d_ms = 0. */
int zpaqhip_gap_hist_blocks_device(zpaqhip_ctx *ctx, const void *d_in, const uint64_t *in_off, size_t n_blocks, uint32_t *hist,
                                   void *hip_stream, zpaqhip_err *err);

#ifdef __cplusplus
}
#endif
#endif
