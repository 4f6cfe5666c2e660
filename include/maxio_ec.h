/*
 * maxio_ec.h — C ABI of the MI355X erasure-coding backend for MaxIO's
 * chunked-EC storage path (src/storage, reference v0.3.2).
 *
 * Plain C: pointers, sizes and int return codes; no C++ types, no torch types,
 * no exceptions cross this boundary.  Every call is reentrant and thread-safe
 * (tokio workers may call concurrently); each device has its own queues.
 * Results are deterministic and independent of the device count.
 *
 * What each entry point replaces in the reference (file:line under the
 * reference checkout; the crates are reed-solomon-erasure 6.0.0 and sha2 0.10.9,
 * Cargo.lock:1462-1473 and :1778-1786):
 *
 *   mxec_rs_check            ReedSolomon::new(k, m) argument errors
 *                            (called at filesystem.rs:1121, chunk_reader.rs:168)
 *   mxec_rs_parity_matrix    the matrix ReedSolomon::new builds (build_matrix)
 *   mxec_sha256_batch        Sha256::digest at filesystem.rs:1070 (write_chunk),
 *                            :1131 (parity), chunk_reader.rs:108 and :184 (verify)
 *   mxec_encode              FilesystemStorage::compute_and_write_parity,
 *                            filesystem.rs:1084-1145 (guard :1095, pad :1108-1113,
 *                            encode :1121-1124, parity digest :1131) plus the data
 *                            digests of write_chunk :1062-1080 — minus the file I/O
 *   mxec_reconstruct         try_reconstruct_data_chunk, chunk_reader.rs:157-226
 *                            (verify :176-196, count :199-208, reconstruct :211,
 *                            truncate :216-222) — minus the file I/O
 *   mxec_*_batch_host        many mxec_encode / mxec_reconstruct calls at once
 *                            from host memory, pipelined over every device
 *   mxec_*_device            the same two operations over device-resident
 *                            batches (objects of any k and chunk size that share
 *                            the output count share one launch)
 *   mxec_write_chunk,
 *   mxec_compute_and_write_parity,
 *   mxec_try_reconstruct_data_chunk,
 *   mxec_put_object_chunked  the file-level functions themselves, writing the
 *                            same `{key}.ec/{index:06}` files and manifest.json
 *                            (filesystem.rs:686-828, 1062-1145; chunk_reader.rs:87-226)
 *   mxec_reader_*            VerifiedChunkReader (chunk_reader.rs:35-85, 228-276)
 *   mxec_body_sums*          the PUT body digests: Md5 ETag + ChecksumHasher
 *                            (filesystem.rs:28-63, 700-725, 775-777)
 *   mxec_frames_*            FrameEncryptor / FrameDecryptor (storage/crypto.rs)
 *                            and the frame AAD builders (filesystem.rs:112-163)
 */
#ifndef MAXIO_EC_H
#define MAXIO_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes -------------------------------------------------------
 * -1..-13 mirror reed_solomon_erasure::Error variants one for one; -14 is the
 * crate's SingularMatrix (matrix.rs); the rest are MaxIO's own guards and this
 * library's device / argument failures. */
#define MXEC_OK 0
#define MXEC_E_TOO_FEW_SHARDS (-1)
#define MXEC_E_TOO_MANY_SHARDS (-2)
#define MXEC_E_TOO_FEW_DATA_SHARDS (-3)
#define MXEC_E_TOO_MANY_DATA_SHARDS (-4)
#define MXEC_E_TOO_FEW_PARITY_SHARDS (-5)
#define MXEC_E_TOO_MANY_PARITY_SHARDS (-6)
#define MXEC_E_TOO_FEW_BUFFER_SHARDS (-7)
#define MXEC_E_TOO_MANY_BUFFER_SHARDS (-8)
#define MXEC_E_INCORRECT_SHARD_SIZE (-9)
#define MXEC_E_TOO_FEW_SHARDS_PRESENT (-10)
#define MXEC_E_EMPTY_SHARD (-11)
#define MXEC_E_INVALID_SHARD_FLAGS (-12)
#define MXEC_E_INVALID_INDEX (-13)
#define MXEC_E_SINGULAR_MATRIX (-14)
#define MXEC_E_TOO_MANY_SHARDS_255 (-20) /* filesystem.rs:1095-1102 k+m>255 */
#define MXEC_E_INVALID_ARG (-21)
#define MXEC_E_DEVICE (-30)
#define MXEC_E_OOM (-31)
#define MXEC_E_NO_DEVICE (-32)
#define MXEC_E_IO (-40)              /* StorageError::Io / io::Error */
#define MXEC_E_INTEGRITY (-41)       /* size or checksum mismatch (InvalidData) */
#define MXEC_E_JSON (-42)            /* StorageError::Json */

/* ---- flags ---------------------------------------------------------------- */
#define MXEC_F_DATA_ONLY 0x1u /* reconstruct: rebuild missing data shards only
                                 (crate reconstruct_data) */

typedef struct mxec_ctx mxec_ctx;

/* ---- library / context ---------------------------------------------------- */
const char* mxec_version(void);
const char* mxec_strerror(int code);
/* Last error message of the calling thread (never NULL). */
const char* mxec_last_error(void);
/* Number of visible HIP devices (0 on a host without a GPU). */
int mxec_device_count(void);
/* device_mask: bit d selects HIP device d; 0 selects every visible device.
 * streams_per_device: HIP streams (and staging rings) per device, >= 1.
 * Returns NULL if no device can be opened (see mxec_last_error). */
mxec_ctx* mxec_open(uint32_t device_mask, int streams_per_device);
/* TEST-ONLY open: as mxec_open, plus settings that exist to drive code paths
 * on a one-GPU test box.  They are never read from the environment, so a
 * production host cannot turn them on by accident.
 *   logical_devices:  open every selected GPU this many times (1..8), each
 *                     copy a separate device with its own streams, arenas,
 *                     combiner and pipeline (the multi-device paths);
 *   rs_grid_cap:      cap every RS launch at this many workgroups (0: off),
 *                     so each workgroup walks many tiles of its grid-stride loop;
 *   coef_arena_bytes: bytes per half of each device's coefficient-table arena
 *                     (0: 64 MiB), small enough that tests recycle it. */
mxec_ctx* mxec_open_test(uint32_t device_mask, int streams_per_device, int logical_devices, uint32_t rs_grid_cap,
                         uint64_t coef_arena_bytes);
void mxec_close(mxec_ctx* ctx);
int mxec_ctx_device_count(const mxec_ctx* ctx);
/* HIP device id of the ctx's i-th device. */
int mxec_ctx_device_id(const mxec_ctx* ctx, int i);
/* Runtime statistics of ctx device i: SHA-256 verification launches run by
 * the device's combiner (concurrent small requests share one launch) and the
 * messages they hashed. */
int mxec_ctx_combiner_stats(mxec_ctx* ctx, int i, uint64_t* launches, uint64_t* messages);
/* Host-batch pipeline (mxec_{encode,reconstruct}_batch_host) counters of ctx
 * device `dev` since the context opened, into out[0 .. n): the copies it
 * issued (1D SDMA DMAs, 2D SDMA DMAs -- the PUT's piece copies -- and their
 * rows, CU-wave copy blocks), the upload brackets MXEC_PIPE_COPY=auto timed
 * and how many ran below its SDMA floor (the rest of those calls' uploads,
 * and the device's for 2 s, copied by waves), the piece-major verified
 * reconstruct waves and the verification groups they ran as, the last timed
 * upload bracket's SDMA rate in MB/s, the same three for downloads
 * (brackets timed, below the floor, last rate), the host-batch calls run on
 * the device and how many of them started while another was in flight, the
 * verified GET's speculative piece rebuilds and the objects it rebuilt
 * again after a verdict, and the host waits that paced a shared call's
 * enqueue.  Returns how many counters were
 * written (min(n, MXEC_PIPE_STAT_COUNT)), or an error.  Diagnostics (tests). */
#define MXEC_PIPE_STAT_COPIES_1D 0
#define MXEC_PIPE_STAT_COPIES_2D 1
#define MXEC_PIPE_STAT_ROWS_2D 2
#define MXEC_PIPE_STAT_WAVE_BLOCKS 3
#define MXEC_PIPE_STAT_SDMA_CHECKS 4
#define MXEC_PIPE_STAT_SDMA_SLOW 5
#define MXEC_PIPE_STAT_VERIFY_WAVES 6
#define MXEC_PIPE_STAT_VERIFY_GROUPS 7
#define MXEC_PIPE_STAT_SDMA_LAST_MBPS 8
#define MXEC_PIPE_STAT_SDMA_DOWN_CHECKS 9
#define MXEC_PIPE_STAT_SDMA_DOWN_SLOW 10
#define MXEC_PIPE_STAT_SDMA_DOWN_LAST_MBPS 11
#define MXEC_PIPE_STAT_CALLS 12
#define MXEC_PIPE_STAT_CALLS_SHARED 13
#define MXEC_PIPE_STAT_SPEC_PIECES 14
#define MXEC_PIPE_STAT_SPEC_REDOS 15
#define MXEC_PIPE_STAT_PACE_WAITS 16
#define MXEC_PIPE_STAT_COUNT 17
int mxec_ctx_pipe_stats(mxec_ctx* ctx, int dev, uint64_t* out, int n);
/* Workgroups per CU the ctx's device `dev` runs large uniform RS launches of
 * (k inputs, m outputs, shard_size) at: the grid tuner times the first
 * launches of a shape at three grid sizes and keeps the fastest (which of
 * them wins depends on the box and on where the batch sits in HBM).  0 while
 * the shape is still being tuned; the default grid for shapes never launched
 * or too small to tune.  Diagnostics (the bench reports it). */
int mxec_ctx_rs_grid(mxec_ctx* ctx, int dev, int k, int m, uint64_t shard_size);
/* Coefficient-table arena statistics of ctx device `dev`: how often the
 * arena's two halves were recycled (a new generation reused the older half),
 * how many batches were queued again because their tables' half was
 * recycled before their launches were fenced, and how many recycles had to
 * wait for a fenced launch still running (fence_waits may be NULL).
 * Diagnostics (tests). */
int mxec_ctx_coef_stats(mxec_ctx* ctx, int dev, uint64_t* recycles, uint64_t* relaunches,
                        uint64_t* fence_waits);
/* Page-locked host memory for request bodies and GET buffers (the Axum body
 * MaxIO hands to a PUT, the buffer a GET fills).  Every host-pointer entry
 * point accepts any host memory; when a buffer comes from here, its bytes
 * move straight to and from the device (by DMA, or by the GPU's own waves
 * over PCIe, INTEGRATION.md MXEC_PIPE_COPY) instead of through the
 * library's pinned staging copy.  NULL on failure; free with
 * mxec_host_free. */
void* mxec_host_alloc(mxec_ctx* ctx, size_t bytes);
/* The same, on the NUMA node of the ctx's device `dev` (MXEC_HOST_NUMA or
 * not): on a host whose GPUs sit on two sockets, a request body meant for a
 * GPU goes on that GPU's socket, and the host batch calls deal an object to
 * a GPU on the node of its pages (pipeline.cpp deal_batch) -- the DMAs then
 * stay off the socket link.  Replaces nothing in the reference (MaxIO's
 * bodies are plain heap memory; filesystem.rs:686-828). */
void* mxec_host_alloc_device(mxec_ctx* ctx, int dev, size_t bytes);
void mxec_host_free(mxec_ctx* ctx, void* p);

/* HBM for a device-resident batch of n_obj objects of (k, m, shard_size),
 * laid out object-major: shard j of object o at
 * base + (o * (k + m) + j) * (*shard_stride), each object's parity after its
 * data -- the layout mxec_encode_strided_device / _reconstruct_strided_device
 * take with obj_stride = (k + m) * shard_stride.  The placement is measured:
 * up to two allocations (the second while the first is held) times two shard
 * strides, each timed by one encode over the whole candidate; the fastest is
 * kept (where a batch lies in HBM moves the encode by up to ~8 %, DESIGN.md
 * §7).  Transiently up to twice the batch's bytes.  probe_ms: NULL, or 4
 * floats receiving the candidates' times (allocation-major; -1 for a
 * candidate not tried).  NULL on failure (mxec_last_error).  Replaces nothing
 * in the reference: a long-lived process allocates its batch buffers once. */
void* mxec_batch_alloc(mxec_ctx* ctx, int dev, int k, int m, uint64_t shard_size,
                       uint64_t n_obj, uint64_t* shard_stride, float* probe_ms);
int mxec_batch_free(mxec_ctx* ctx, void* p);

/* ---- ReedSolomon::new ----------------------------------------------------- */
/* 0 if new(k, m) would succeed; otherwise the crate's error
 * (TooFewDataShards / TooFewParityShards / TooManyShards). */
int mxec_rs_check(int k, int m);
/* Writes the m x k parity rows of the crate's encoding matrix, row-major. */
int mxec_rs_parity_matrix(int k, int m, uint8_t* out);

/* ---- host-pointer entry points (the drop-in for one request) -------------- */
/* SHA-256 of n host buffers; out[i] = digest of bufs[i][0..lens[i]). */
int mxec_sha256_batch(mxec_ctx* ctx, const uint8_t* const* bufs,
                      const size_t* lens, size_t n, uint8_t (*out)[32]);

/* Encode one object: k data chunks (data_len[j] <= shard_size bytes, zero
 * padded to shard_size as filesystem.rs:1111 does), m parity outputs of
 * shard_size bytes each.  sha256_out, if not NULL, receives k+m digests:
 * data digests over the unpadded bytes (write_chunk :1070), parity digests over
 * the full shard (:1131).  data_len NULL means every chunk is shard_size. */
int mxec_encode(mxec_ctx* ctx, int k, int m, size_t shard_size,
                const uint8_t* const* data, const size_t* data_len,
                uint8_t* const* parity, uint8_t (*sha256_out)[32]);

/* Reconstruct one object, try_reconstruct_data_chunk semantics.
 * shards[i] (i < k+m) holds shard_len[i] bytes when present_inout[i] != 0;
 * for a missing shard it is the output buffer (shard_len[i] bytes; parity
 * shards use shard_size).  If expected_sha256 is not NULL every present shard
 * is hashed and a mismatch turns it into an erasure (:176-196), rebuilt into
 * the same buffer at shard_len[i] bytes.  Missing
 * shards are rebuilt (all of them, or data only with MXEC_F_DATA_ONLY);
 * present_inout[i] is 1 on return for every verified or rebuilt shard.
 * Fewer than k verified shards: MXEC_E_TOO_FEW_SHARDS_PRESENT, nothing is
 * written, and *n_present (if not NULL) holds the verified count.
 * Shape: this and every other reconstruct entry point take what
 * ReedSolomon::new takes, k + m <= 256 (mxec_rs_check), so a stripe of 256
 * shards written elsewhere is rebuilt like any other, shard index 255 among
 * the missing or among the inputs (tests/test_wide_stripes_gpu.py); 257 and
 * more are MXEC_E_TOO_MANY_SHARDS.  The encodes, verifies and locates stop
 * at k + m = 255 with MXEC_E_TOO_MANY_SHARDS_255, as filesystem.rs:1095
 * does, so no 256-shard stripe comes from this library. */
int mxec_reconstruct(mxec_ctx* ctx, int k, int m, size_t shard_size,
                     uint8_t* const* shards, const size_t* shard_len,
                     const uint8_t (*expected_sha256)[32],
                     uint8_t* present_inout, uint32_t flags, int* n_present);

/* ---- completion handles (non-blocking host calls) -------------------------
 * The *_async forms queue the blocking call of the same name on the
 * context's worker threads and return at once (MXEC_OK and *ticket set), or
 * return an argument error without a ticket.  Pointer arrays, digests to
 * compare and directory strings are copied at submission; data buffers and
 * out-parameters (parity, shards, present_inout, n_present, out, out_len)
 * must stay valid until the ticket completes.  A tokio caller registers
 * mxec_ticket_fd (an eventfd, readable once the call is done) with AsyncFd
 * and awaits it instead of parking a blocking-pool thread for the ~30 ms a
 * 1 MiB chunk's SHA-256 chain takes (chunk_reader.rs:244-249, main.rs:81). */
typedef struct mxec_ticket mxec_ticket;
/* eventfd that becomes readable when the call completes. */
int mxec_ticket_fd(const mxec_ticket* t);
/* 1 when complete, 0 while running (never blocks). */
int mxec_ticket_poll(mxec_ticket* t);
/* Blocks until complete; returns the call's status and sets the calling
 * thread's mxec_last_error to its message. */
int mxec_ticket_wait(mxec_ticket* t);
/* The failed call's message ("" on success or while running). */
const char* mxec_ticket_error(const mxec_ticket* t);
/* Waits for completion if needed, then frees the ticket and its fd. */
void mxec_ticket_free(mxec_ticket* t);
int mxec_sha256_batch_async(mxec_ctx* ctx, const uint8_t* const* bufs, const size_t* lens,
                            size_t n, uint8_t (*out)[32], mxec_ticket** ticket);
int mxec_encode_async(mxec_ctx* ctx, int k, int m, size_t shard_size,
                      const uint8_t* const* data, const size_t* data_len,
                      uint8_t* const* parity, uint8_t (*sha256_out)[32], mxec_ticket** ticket);
int mxec_reconstruct_async(mxec_ctx* ctx, int k, int m, size_t shard_size,
                           uint8_t* const* shards, const size_t* shard_len,
                           const uint8_t (*expected_sha256)[32], uint8_t* present_inout,
                           uint32_t flags, int* n_present, mxec_ticket** ticket);
int mxec_put_object_chunked_async(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                  uint32_t parity_shards, const uint8_t* body, size_t len,
                                  mxec_ticket** ticket);
int mxec_get_object_chunked_async(mxec_ctx* ctx, const char* ec_dir, uint64_t offset,
                                  uint64_t length, uint8_t* out, uint64_t out_cap,
                                  uint64_t* out_len, mxec_ticket** ticket);

/* ---- device-resident batches ---------------------------------------------
 * All data pointers below are HIP device pointers on ctx device `dev`
 * (index into the ctx's devices).  `stream` is a hipStream_t of that device;
 * NULL is the HIP null (default) stream, as in other HIP libraries, so work
 * the caller queued there is ordered before ours.  Calls return after
 * enqueueing, except
 * mxec_reconstruct_strided_device and mxec_reconstruct_batch_device with
 * verification, which synchronise once to read the verdicts (the erasure
 * pattern picks the decode matrix). */

/* Uniform batch of n_obj objects, each k data + m parity shards of
 * shard_size bytes.  Object o, data shard j lives at
 * data + o*data_obj_stride + j*data_shard_stride (likewise parity).
 * data_len (host, k entries, NULL = shard_size) applies to every object.
 * digests_dev (device, n_obj*(k+m)*32, NULL = skip) gets the data then
 * parity digests of each object, object-major. */
int mxec_encode_strided_device(mxec_ctx* ctx, int dev, void* stream, int k,
                               int m, uint64_t shard_size, uint64_t n_obj,
                               const uint8_t* data, uint64_t data_obj_stride,
                               uint64_t data_shard_stride,
                               const uint64_t* data_len, uint8_t* parity,
                               uint64_t parity_obj_stride,
                               uint64_t parity_shard_stride,
                               uint8_t* digests_dev);

/* Running parity over a window of the data shards (a streaming PUT folds
 * chunks in as they arrive; the crate computes parity only once every chunk
 * is on disk, filesystem.rs:1121-1124, so this call replaces nothing in it):
 * parity_out = parity_in ^ M(k,m)[:, first .. first+count) * data window, per
 * object.  data points at shard `first` of object 0 (only the window need be
 * resident); data_len: host, `count` entries, NULL = shard_size.  parity_in
 * NULL: zeros (the first window).  parity_in and parity_out must not overlap
 * (MXEC_E_INVALID_ARG): the pass reads one and writes the other, never one
 * buffer in place.  Enqueue-only.  After windows that together cover [0, k)
 * exactly once, in any order, parity_out holds mxec_encode_strided_device's
 * parity.  Each update moves (count + 2m) * shard_size bytes per object.
 * (k, m) and shard-size errors are mxec_encode_strided_device's; first < 0,
 * count < 1, first + count > k, a null data or parity_out and overlapping
 * in / out rows are MXEC_E_INVALID_ARG, all decided before anything is
 * enqueued. */
int mxec_encode_update_strided_device(mxec_ctx* ctx, int dev, void* stream, int k,
                                      int m, uint64_t shard_size, uint64_t n_obj,
                                      int first, int count, const uint8_t* data,
                                      uint64_t data_obj_stride, uint64_t data_shard_stride,
                                      const uint64_t* data_len, const uint8_t* parity_in,
                                      uint64_t in_obj_stride, uint64_t in_shard_stride,
                                      uint8_t* parity_out, uint64_t out_obj_stride,
                                      uint64_t out_shard_stride);

/* General batch: object o has k[o] data and m[o] parity shards of
 * shard_size[o] bytes; the pointer arrays are host arrays of device pointers,
 * concatenated over objects (sum k, sum m entries); data_len likewise (NULL =
 * full shards).  digests_dev: sum(k+m)*32 bytes, object-major, or NULL.
 * Objects with the same m share one kernel launch whatever their k and
 * shard size (16-byte aligned pointers, m <= 8; otherwise one launch per
 * (k, m, shard_size)). */
typedef struct mxec_object {
    int32_t k;
    int32_t m;
    uint64_t shard_size;
} mxec_object;
int mxec_encode_batch_device(mxec_ctx* ctx, int dev, void* stream,
                             const mxec_object* objs, uint64_t n_obj,
                             const uint8_t* const* data,
                             const uint64_t* data_len,
                             uint8_t* const* parity, uint8_t* digests_dev);

/* ---- ReedSolomon::verify --------------------------------------------------
 * Recomputes the parity of the data shards on the GPU and compares it with
 * the stored parity there: (k + m) * shard_size bytes read per object, none
 * written, no parity downloaded.  A row's result is the lowest byte offset
 * within the shard at which the stored row differs from the recomputed one,
 * or MXEC_VERIFY_OK when they agree.  Data shorter than shard_size counts as
 * zero padded (filesystem.rs:1111) and is not read past its length.
 * Argument and (k, m) errors are mxec_encode's; m == 0 is
 * MXEC_E_TOO_FEW_PARITY_SHARDS, as ReedSolomon::new gives. */
#define MXEC_VERIFY_OK UINT64_MAX
/* One object in host memory, through mxec_encode's one-request path: the
 * shards go up, m * 8 bytes come back.  parity[i]: shard_size bytes.
 * first_bad: m entries, may be NULL.  *consistent (may be NULL): 1 iff every
 * row matches -- the crate's verify() result. */
int mxec_verify(mxec_ctx* ctx, int k, int m, size_t shard_size,
                const uint8_t* const* data, const size_t* data_len,
                const uint8_t* const* parity, uint64_t* first_bad, int* consistent);
/* Device-resident batches, laid out as mxec_encode_strided_device /
 * mxec_encode_batch_device take them; enqueue-only like those.  first_bad_dev
 * is a device array of n_obj * m (strided) or sum(m) (batch) entries,
 * object-major, filled on `stream` ahead of the kernel: read it after the
 * stream has drained.  Objects of a batch that share m share one launch. */
int mxec_verify_strided_device(mxec_ctx* ctx, int dev, void* stream, int k,
                               int m, uint64_t shard_size, uint64_t n_obj,
                               const uint8_t* data, uint64_t data_obj_stride,
                               uint64_t data_shard_stride,
                               const uint64_t* data_len, const uint8_t* parity,
                               uint64_t parity_obj_stride,
                               uint64_t parity_shard_stride,
                               uint64_t* first_bad_dev);
int mxec_verify_batch_device(mxec_ctx* ctx, int dev, void* stream,
                             const mxec_object* objs, uint64_t n_obj,
                             const uint8_t* const* data,
                             const uint64_t* data_len,
                             const uint8_t* const* parity,
                             uint64_t* first_bad_dev);

/* ---- locate: which shard is damaged, from the parity alone -----------------
 * The verify's walk, but on a mismatch every bad byte column (one whose m
 * syndrome bytes s_i = stored_parity_i ^ recomputed_parity_i are not all
 * zero) is classified.  Exactly one s_i non-zero: parity shard k + i.  All m
 * non-zero and s = M[:, j] * e for one data shard j whose length reaches the
 * column: data shard j.  Anything else fits no single shard:
 * MXEC_LOCATE_NO_SHARD.  The encoding matrix is MDS, so a corruption confined
 * to one shard is named uniquely, column by column.  Needs 2 <= m <= 8: one
 * parity row cannot tell shards apart, more than eight do not fit the
 * kernel's one row block (MXEC_E_INVALID_ARG; m == 0 is
 * MXEC_E_TOO_FEW_PARITY_SHARDS); every other error is the verify's, and
 * all are decided before anything is enqueued.  A clean stripe costs what
 * the verify costs and writes nothing. */
#define MXEC_LOCATE_NO_SHARD 0xFFFFFFFEu
struct mxec_locate_result {
    uint64_t first_bad; /* lowest bad byte column, MXEC_VERIFY_OK if none */
    uint64_t n_bad;     /* number of bad byte columns */
    uint32_t shard_min; /* min / max over the bad columns' candidates (shard */
    uint32_t shard_max; /*   index or MXEC_LOCATE_NO_SHARD); clean: UINT32_MAX / 0 */
};
typedef struct mxec_locate_result mxec_locate_result;
/* What a result amounts to (pure host function, no context):
 * MXEC_LOCATE_CLEAN (n_bad == 0), _ONE (shard_min == shard_max < 256;
 * *shard, if not NULL, receives it), _MANY (everything else).  `result`
 * points at a mxec_locate_result. */
#define MXEC_LOCATE_CLEAN 0
#define MXEC_LOCATE_ONE 1
#define MXEC_LOCATE_MANY 2
int mxec_locate_outcome(const void* result, uint32_t* shard);
/* One object in host memory, through the host verify's one-request path: the
 * shards go up, 24 bytes come back.  `out` points at a mxec_locate_result. */
int mxec_locate(mxec_ctx* ctx, int k, int m, size_t shard_size,
                const uint8_t* const* data, const size_t* data_len,
                const uint8_t* const* parity, void* out);
/* Device-resident batches, laid out and enqueued as the verify's.  out_dev is
 * a device array of n_obj mxec_locate_result records, initialised on `stream`
 * ahead of the kernel and filled by it: read it after the stream has
 * drained.  Objects of a batch that share m share one launch. */
int mxec_locate_strided_device(mxec_ctx* ctx, int dev, void* stream, int k,
                               int m, uint64_t shard_size, uint64_t n_obj,
                               const uint8_t* data, uint64_t data_obj_stride,
                               uint64_t data_shard_stride,
                               const uint64_t* data_len, const uint8_t* parity,
                               uint64_t parity_obj_stride,
                               uint64_t parity_shard_stride, void* out_dev);
int mxec_locate_batch_device(mxec_ctx* ctx, int dev, void* stream,
                             const mxec_object* objs, uint64_t n_obj,
                             const uint8_t* const* data,
                             const uint64_t* data_len,
                             const uint8_t* const* parity, void* out_dev);

/* End-to-end PUT compute for many objects whose chunks are in HOST memory
 * (request bodies) — the batched form of mxec_encode.  Same array layout as
 * mxec_encode_batch_device but host pointers; digests (host, sum(k+m)) and
 * status_out (host, n_obj) may be NULL.  Objects are dealt over the ctx's
 * devices -- object o to device o mod D when every object has the same
 * (k, m, shard_size), balanced by bytes otherwise; per device, uploads
 * (direct from pinned memory, else via a pinned ring), RS + SHA-256 kernels
 * and downloads are pipelined on separate streams with the whole batch
 * resident in HBM.  Blocks until every
 * parity chunk and digest is in host memory.  Thread-safe: concurrent
 * calls (this one and mxec_reconstruct_batch_host, from any threads) share
 * each device -- up to MXEC_PIPE_LANES at once, their waves interleaved on
 * the device's four pipeline streams. */
int mxec_encode_batch_host(mxec_ctx* ctx, const mxec_object* objs,
                           uint64_t n_obj, const uint8_t* const* data,
                           const uint64_t* data_len, uint8_t* const* parity,
                           uint8_t (*digests)[32], int32_t* status_out);

/* End-to-end GET compute for many objects whose shards are in HOST memory
 * (the shard files as read from disk) -- the batched form of
 * mxec_reconstruct (try_reconstruct_data_chunk, chunk_reader.rs:157-226, per
 * object).  Same array layout as mxec_reconstruct_batch_device but host
 * pointers: shards (sum(k+m), object-major; a missing shard's pointer is the
 * buffer its rebuilt bytes go to), shard_len (NULL = shard_size), present
 * (in/out); expected_sha256 (host, sum(k+m) digests) or NULL to skip
 * verification; status_out (host, n_obj) may be NULL.  Objects are dealt
 * over the ctx's devices as mxec_encode_batch_host deals them; per device the
 * present shards go up (direct from pinned memory, else via a pinned ring),
 * are verified and rebuilt there, and only the rebuilt shards come back.  With
 * verification the missing shards are rebuilt piece by piece as the present
 * ones arrive, before the verdict (MXEC_GET_SPECULATE, default on), and an
 * object whose verdict drops a shard is rebuilt again from the verified
 * ones.  An object short of k verified shards gets
 * MXEC_E_TOO_FEW_SHARDS_PRESENT: its present shards' buffers are not written
 * and its missing shards' buffers are undefined (not written with
 * MXEC_GET_SPECULATE=0; the reference returns an error and no data,
 * chunk_reader.rs:203-206); the call returns the first such status.
 * Blocks until every rebuilt shard is in host memory.  Thread-safe, as
 * mxec_encode_batch_host. */
int mxec_reconstruct_batch_host(mxec_ctx* ctx, const mxec_object* objs,
                                uint64_t n_obj, uint8_t* const* shards,
                                const uint64_t* shard_len, uint8_t* present,
                                const uint8_t (*expected_sha256)[32],
                                uint32_t flags, int32_t* status_out);

/* Uniform reconstruct batch.  Object o, shard i (0 <= i < k+m) lives at
 * shards + o*obj_stride + i*shard_stride.  shard_len (host, k+m entries,
 * NULL = shard_size) is the byte length of shard i in every object.
 * present (host, n_obj*(k+m)) in/out as in mxec_reconstruct.
 * expected_sha_dev (device, n_obj*(k+m)*32) or NULL to skip verification.
 * status_out (host, n_obj, may be NULL): 0 or MXEC_E_TOO_FEW_SHARDS_PRESENT
 * per object; the call returns the first non-zero status.  With verification
 * the rebuild from the mask as given runs beside the hash (objects with a
 * digest mismatch are rebuilt again), so an object that fails may have had
 * its missing shards written. */
int mxec_reconstruct_strided_device(mxec_ctx* ctx, int dev, void* stream,
                                    int k, int m, uint64_t shard_size,
                                    uint64_t n_obj, uint8_t* shards,
                                    uint64_t obj_stride, uint64_t shard_stride,
                                    const uint64_t* shard_len, uint8_t* present,
                                    const uint8_t* expected_sha_dev,
                                    uint32_t flags, int32_t* status_out);

/* The completion-handle form (see mxec_ticket above): shard_len is copied at
 * submission; present and status_out must stay valid until the ticket
 * completes, and the shards are the caller's until then. */
int mxec_reconstruct_strided_device_async(mxec_ctx* ctx, int dev, void* stream,
                                          int k, int m, uint64_t shard_size,
                                          uint64_t n_obj, uint8_t* shards,
                                          uint64_t obj_stride, uint64_t shard_stride,
                                          const uint64_t* shard_len, uint8_t* present,
                                          const uint8_t* expected_sha_dev,
                                          uint32_t flags, int32_t* status_out,
                                          mxec_ticket** ticket);

/* Mixed reconstruct batch — the counterpart of mxec_encode_batch_device for
 * a stream of objects of different (k, m) and shard sizes (BASELINE
 * configs[4]; try_reconstruct_data_chunk, chunk_reader.rs:157-226, per
 * object).  shards (host array of device pointers, sum(k+m) entries,
 * object-major), shard_len (host, sum(k+m), NULL = shard_size) and present
 * (host, sum(k+m), in/out as in mxec_reconstruct) are concatenated over
 * objects; expected_sha_dev (device, sum(k+m)*32) or NULL to skip
 * verification; status_out (host, n_obj, may be NULL) as in
 * mxec_reconstruct_strided_device.  With verification the call synchronises
 * once to read the verdicts.  Objects of every shape that rebuild the same
 * number of shards share one kernel launch. */
int mxec_reconstruct_batch_device(mxec_ctx* ctx, int dev, void* stream,
                                  const mxec_object* objs, uint64_t n_obj,
                                  uint8_t* const* shards,
                                  const uint64_t* shard_len, uint8_t* present,
                                  const uint8_t* expected_sha_dev,
                                  uint32_t flags, int32_t* status_out);

/* The completion-handle form: objs, shards and shard_len are copied at
 * submission; present and status_out must stay valid until the ticket
 * completes, and the shards are the caller's until then. */
int mxec_reconstruct_batch_device_async(mxec_ctx* ctx, int dev, void* stream,
                                        const mxec_object* objs, uint64_t n_obj,
                                        uint8_t* const* shards,
                                        const uint64_t* shard_len,
                                        uint8_t* present,
                                        const uint8_t* expected_sha_dev,
                                        uint32_t flags, int32_t* status_out,
                                        mxec_ticket** ticket);

/* SHA-256 of n device buffers (host arrays of device pointers and lengths)
 * into digests_dev (device, n*32). */
int mxec_sha256_batch_device(mxec_ctx* ctx, int dev, void* stream,
                             const uint8_t* const* bufs, const uint64_t* lens,
                             uint64_t n, uint8_t* digests_dev);

/* ---- file-level path (src/storage/filesystem.rs, chunk_reader.rs) -------- */
/* ChunkInfo (mod.rs:182-189): kind 0 = data, 1 = parity. */
typedef struct mxec_chunk_info {
    uint32_t index;
    uint64_t size;
    char sha256[65]; /* lowercase hex + NUL, hex::encode(Sha256::digest) */
    uint8_t kind;
} mxec_chunk_info;

/* write_chunk (filesystem.rs:1062-1080): writes ec_dir/{index:06}. */
int mxec_write_chunk(mxec_ctx* ctx, const char* ec_dir, uint32_t index,
                     const uint8_t* data, size_t len, mxec_chunk_info* out);

/* compute_and_write_parity (filesystem.rs:1084-1145): re-reads the k data
 * chunk files named by data_chunks, encodes, writes ec_dir/{k+i:06}. */
int mxec_compute_and_write_parity(mxec_ctx* ctx, const char* ec_dir,
                                  uint64_t chunk_size, uint32_t parity_shards,
                                  const mxec_chunk_info* data_chunks, int k,
                                  mxec_chunk_info* parity_out);

/* put_object_chunked's chunking + manifest (filesystem.rs:686-773) for a
 * fully buffered body: chunks of chunk_size, empty body -> one empty chunk and
 * no parity, parity when parity_shards > 0 && len > 0, manifest.json written
 * with serde_json::to_string_pretty's layout. */
int mxec_put_object_chunked(mxec_ctx* ctx, const char* ec_dir,
                            uint64_t chunk_size, uint32_t parity_shards,
                            const uint8_t* body, size_t len);

/* ---- encrypt-then-EC frames (src/storage/crypto.rs, filesystem.rs:112-163) --
 * The object body is cut into frame_size (FRAME_CHUNK_SIZE = 65536) plaintext
 * frames; frame i is nonce(12) = prefix(4) || (first_index + i) as u64 LE,
 * then the AES-256-GCM ciphertext, then the 16-byte tag (crypto.rs:1-20,
 * 426-432).  The EC layer then chunks these bytes like any body.
 * aad: NULL with aad_len 0 (no_aad), or n_frames * aad_len bytes with frame
 * i's AAD at aad + i * aad_len (mxec_frame_aads builds the reference's
 * SHA-256(identity || index LE) AADs).                                      */
#define MXEC_FRAME_CHUNK_SIZE 65536u
#define MXEC_FRAME_OVERHEAD 28u
/* Bytes of the frame stream for plaintext_len bytes. */
uint64_t mxec_frames_len(uint64_t plaintext_len, uint32_t frame_size);
/* FrameEncryptor over a whole buffer; out receives mxec_frames_len bytes. */
int mxec_frames_encrypt(mxec_ctx* ctx, const uint8_t key[32], const uint8_t nonce_prefix[4],
                        uint64_t first_index, const uint8_t* aad, uint32_t aad_len,
                        uint32_t frame_size, const uint8_t* pt, uint64_t len,
                        uint8_t* out, uint64_t out_cap, uint64_t* out_len);
/* FrameDecryptor over a whole buffer: every frame's stored index and tag are
 * checked (MXEC_E_INTEGRITY with crypto.rs's messages: "frame index mismatch:
 * expected E, got G", "AES-GCM decryption failed: authentication error",
 * "truncated encrypted frame"); no plaintext is returned on failure. */
int mxec_frames_decrypt(mxec_ctx* ctx, const uint8_t key[32], uint64_t first_index,
                        const uint8_t* aad, uint32_t aad_len, uint32_t frame_size,
                        const uint8_t* frames, uint64_t frames_len, uint64_t plaintext_size,
                        uint8_t* out, uint64_t out_cap, uint64_t* out_len);
/* Device-resident batches: one launch over every frame of every job.
 * Pointer contract: in_dev, out_dev and aad_dev may have any byte alignment.
 * A payload sits 12 bytes into its frame and frames are frame_size + 28 bytes
 * apart, so the two sides of a copy are never 16-byte aligned together; the
 * kernel declares no alignment on its 16-byte accesses and gfx950 serves
 * global memory unaligned.  Nothing is rejected for its alignment.  The
 * buffers of one call must not overlap.                                      */
typedef struct mxec_frames_job {
    const uint8_t* key;       /* host, 32 bytes */
    uint8_t nonce_prefix[4];  /* encrypt only */
    uint32_t frame_size;
    uint64_t first_index;
    const uint8_t* aad_dev;   /* device, n_frames * aad_len bytes, or NULL */
    uint32_t aad_len;
    uint32_t reserved;
    const uint8_t* in_dev;    /* encrypt: plaintext; decrypt: frame stream */
    uint64_t len;             /* plaintext bytes */
    uint8_t* out_dev;         /* encrypt: frame stream; decrypt: plaintext */
} mxec_frames_job;
int mxec_frames_encrypt_device(mxec_ctx* ctx, int dev, void* stream,
                               const mxec_frames_job* jobs, uint64_t n_jobs);
/* Synchronous; status_out[j] = 0 or MXEC_E_INTEGRITY per job. */
int mxec_frames_decrypt_device(mxec_ctx* ctx, int dev, void* stream,
                               const mxec_frames_job* jobs, uint64_t n_jobs,
                               int32_t* status_out);
/* The encrypt form whose destination is a ring of chunk slots instead of one
 * contiguous run: FrameEncryptor (crypto.rs:94-117) writing straight into the
 * chunks put_object_chunked_encrypted's loop cuts its output into
 * (filesystem.rs:835-1060).  Byte x of the frame stream is stored at
 *     base_dev + ((x / chunk_size) % slots) * slot_stride + x % chunk_size.
 * One job per call; job->out_dev is ignored.  stream_off is the frame-stream
 * offset of the job's first frame and may take any value.  A frame's nonce,
 * ciphertext and tag may each be cut by chunk boundaries, any number of times,
 * and by the ring's wrap.  Bytes of the window outside the mapped range (the
 * slot_stride - chunk_size gaps, the other slots) are never written.
 * Enqueue-only on `stream`.  MXEC_E_INVALID_ARG, decided before anything is
 * queued: a null job, win, key, base_dev, in_dev with len > 0 or aad_dev with
 * aad_len > 0; a frame_size that is 0, no multiple of 16 or above 2^31 - 256;
 * chunk_size == 0; slot_stride < chunk_size; slots == 0 or a window of 2^62
 * bytes or more; a job whose stream bytes (mxec_frames_len) span more than
 * slots * chunk_size, for it would overwrite itself.  len == 0 is MXEC_OK and
 * does nothing.  `win` points at a mxec_frames_window, passed as const void*
 * (as mxec_scrub_object passes its report). */
struct mxec_frames_window {
    uint8_t* base_dev;      /* slot 0 */
    uint64_t chunk_size;    /* frame-stream bytes per chunk, > 0 */
    uint64_t slot_stride;   /* >= chunk_size */
    uint64_t slots;         /* >= 1; chunk j lives in slot j % slots */
};
typedef struct mxec_frames_window mxec_frames_window;
int mxec_frames_encrypt_window_device(mxec_ctx* ctx, int dev, void* stream,
                                      const mxec_frames_job* job, uint64_t stream_off,
                                      const void* win);
/* The decrypt form whose source is that ring: FrameDecryptor (crypto.rs:186-420)
 * reading verified chunks where they lie in HBM.  Byte x of the frame stream is
 * read from base_dev + ((x / chunk_size) % slots) * slot_stride + x % chunk_size;
 * job->out_dev receives job->len plaintext bytes, contiguous.  One job per
 * call; job->in_dev and job->nonce_prefix are ignored.  frame_status_dev is a
 * device array of one int32_t per frame: 0 ok, 1 tag mismatch, 2 the stored
 * index is not first_index + f (an index mismatch takes precedence).  The
 * plaintext of a frame whose status is not 0 is in out_dev all the same and
 * must not be used.  A stored nonce, ciphertext and tag may each be cut by
 * chunk boundaries, any number of times, and by the ring's wrap.  Bytes of the
 * window outside the mapped range are never read; nothing but out_dev[0, len)
 * and the statuses is written.  Enqueue-only on `stream`, statuses included:
 * unlike mxec_frames_decrypt_device it does not wait, so a caller queues its
 * downloads behind it.  MXEC_E_INVALID_ARG, decided before anything is queued:
 * what mxec_frames_encrypt_window_device refuses (with out_dev in the place of
 * in_dev), a null frame_status_dev with len > 0, and a job whose stream bytes
 * exceed the window's slots * chunk_size, for its first bytes would no longer
 * be resident.  len == 0 is MXEC_OK and does nothing. */
int mxec_frames_decrypt_window_device(mxec_ctx* ctx, int dev, void* stream,
                                      const mxec_frames_job* job, uint64_t stream_off,
                                      const void* win, int32_t* frame_status_dev);
/* The decrypt form whose plaintext side is a byte ring: FrameDecryptor
 * (crypto.rs:186-420) over the frames of multipart parts, writing straight into
 * the plaintext ring a streaming re-encryption reads
 * (complete_multipart_chunked_encrypted, filesystem.rs:1375-1387).  Any number
 * of jobs, each with its own key, AADs and first_index; jobs[j].in_dev is job
 * j's contiguous frame stream from first_index on, jobs[j].out_dev and
 * nonce_prefix are ignored.  Plaintext byte o of job j is stored at
 *     base_dev + (ring_off[j] + o) % bytes,
 * so a job may start at any byte of the ring and the ring's wrap may cut a
 * frame anywhere: inside a 16-byte block, on a block or frame boundary, in the
 * partial last block.  frame_status_dev is a device array of one int32_t per
 * frame, in job order: 0 ok, 1 tag mismatch, 2 the stored index is not
 * first_index + f (an index mismatch takes precedence).  The plaintext of a
 * frame whose status is not 0 is in the ring all the same and must not be
 * used.  Nothing past base_dev + bytes and nothing in the ring outside the
 * jobs' ranges is written.  The ranges of one call must not overlap: that is
 * the caller's contract.  Enqueue-only on `stream`, statuses included.
 * MXEC_E_INVALID_ARG, decided before anything is queued: a null jobs with
 * n_jobs > 0; a null ring, base_dev, ring_off, key, in_dev with len > 0 or
 * aad_dev with aad_len > 0; bytes == 0; a ring_off[j] >= bytes; a frame_size
 * that is 0, no multiple of 16 or above 2^31 - 256; a null frame_status_dev
 * when a job has frames; the jobs' len summing to more than bytes, for the call
 * would overwrite itself.  n_jobs == 0, or every len == 0, is MXEC_OK and does
 * nothing.  `ring` points at a mxec_frames_ring, passed as const void*. */
struct mxec_frames_ring {
    uint8_t* base_dev;      /* byte 0 of the ring, any alignment */
    uint64_t bytes;         /* > 0, any value                    */
};
typedef struct mxec_frames_ring mxec_frames_ring;
int mxec_frames_decrypt_ring_device(mxec_ctx* ctx, int dev, void* stream,
                                    const mxec_frames_job* jobs, uint64_t n_jobs,
                                    const uint64_t* ring_off, const void* ring,
                                    int32_t* frame_status_dev);
/* build_frame_aad / build_part_aad (filesystem.rs:118-158): out[i] =
 * SHA-256(prefix || (first_index + i) as u64 LE), prefix = the identity bytes
 * (bucket 0 key 0 version 0, or "PART" 0 upload_id 0 part_le4 0). */
int mxec_frame_aads(mxec_ctx* ctx, const uint8_t* prefix, uint32_t prefix_len,
                    uint64_t first_index, uint64_t n_frames, uint8_t (*out)[32]);

/* ---- PUT body digests (filesystem.rs:28-63, 700-725, 775-777) -------------
 * Every PUT hashes the whole body with MD5 (the ETag, hex-encoded and quoted
 * by the caller) and, when the request names an algorithm, with the
 * ChecksumHasher (x-amz-checksum-*, base64 of the bytes below).              */
#define MXEC_SUM_MD5    0x01u
#define MXEC_SUM_CRC32  0x02u /* crc32fast::Hasher::finalize               */
#define MXEC_SUM_CRC32C 0x04u /* crc32c::crc32c_append(0, body)            */
#define MXEC_SUM_SHA1   0x08u
#define MXEC_SUM_SHA256 0x10u
typedef struct mxec_body_sums {
    uint8_t md5[16];
    uint32_t crc32;  /* the u32 value; to_be_bytes() before base64 */
    uint32_t crc32c;
    uint8_t sha1[20];
    uint8_t sha256[32];
} mxec_body_sums;    /* 76 bytes; fields not requested are left untouched */

/* Digests of n host bodies (one record each). */
int mxec_body_sums_batch(mxec_ctx* ctx, const uint8_t* const* bodies, const uint64_t* lens,
                         uint64_t n, uint32_t which, mxec_body_sums* out);
/* Device-resident bodies (host array of device pointers); out_dev is a device
 * array of n records, written asynchronously on `stream`. */
int mxec_body_sums_batch_device(mxec_ctx* ctx, int dev, void* stream,
                                const uint8_t* const* bodies_dev, const uint64_t* lens,
                                uint64_t n, uint32_t which, mxec_body_sums* out_dev);
/* The same digests over bodies that arrive in pieces: replaces Md5::update /
 * ChecksumHasher::update per stream piece (filesystem.rs:722-725) and their
 * finalize (:775-777).  There are n bodies; body i's running state is the
 * record at state_dev + i * MXEC_SUMS_STATE_BYTES, device memory of the
 * caller's (16-byte aligned, layout private to the library) that need not be
 * initialised before a FIRST call: FIRST starts every body from scratch,
 * whatever its record holds.  Each call takes the next piece of every body
 * (host array of device pointers, any length including 0, any alignment; a
 * pointer may be NULL when its length is 0) and is enqueue-only on `stream`:
 * no call waits for the GPU, so pieces may come and go through a bounded
 * window.  Calls on one record must be stream-ordered and use the same
 * `which`.  With FINAL, out_dev[i] receives exactly what
 * mxec_body_sums_batch_device writes for the concatenation of body i's pieces
 * since FIRST (fields not requested are left untouched); FIRST | FINAL in one
 * call is that call.  out_dev is read only with FINAL and may be NULL
 * otherwise.  MXEC_E_INVALID_ARG, decided before anything is enqueued: unknown
 * `which` or `flags` bits, a null or misaligned state_dev, a null out_dev
 * with FINAL, a null piece of non-zero length.  n == 0 or which == 0 is
 * MXEC_OK and does nothing. */
#define MXEC_SUMS_STATE_BYTES 512u
#define MXEC_SUMS_F_FIRST 1u
#define MXEC_SUMS_F_FINAL 2u
int mxec_body_sums_update_device(mxec_ctx* ctx, int dev, void* stream,
                                 const uint8_t* const* pieces_dev, const uint64_t* lens,
                                 uint64_t n, uint32_t which, uint32_t flags,
                                 void* state_dev, mxec_body_sums* out_dev);
/* put_object_chunked plus the body digests it computes on the way
 * (PutResult etag / checksum_value, filesystem.rs:775-777). */
int mxec_put_object_chunked_sums(mxec_ctx* ctx, const char* ec_dir,
                                 uint64_t chunk_size, uint32_t parity_shards,
                                 const uint8_t* body, size_t len, uint32_t which,
                                 mxec_body_sums* sums_out);

/* put_object_chunked_encrypted (filesystem.rs:835-1060) for a buffered body:
 * the plaintext becomes AES-256-GCM 64 KiB frames (first index 0, frame i's
 * AAD = SHA-256(aad_prefix || i LE) with aad_prefix = bucket 0 key 0
 * version 0, build_frame_aad :118-128), the frame stream is chunked, parity
 * added, and manifest.json records total_size = frame-stream bytes and
 * plaintext_size.  `which` / sums_out: the plaintext body digests as in
 * mxec_put_object_chunked_sums (0 / NULL to skip). */
int mxec_put_object_chunked_encrypted(mxec_ctx* ctx, const char* ec_dir,
                                      uint64_t chunk_size, uint32_t parity_shards,
                                      const uint8_t key[32], const uint8_t nonce_prefix[4],
                                      const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                                      const uint8_t* body, size_t len, uint32_t which,
                                      mxec_body_sums* sums_out);

/* One part of a CompleteMultipartUpload (PartMeta, multipart.rs). */
typedef struct mxec_multipart_part {
    const char* path;      /* part file (upload_part wrote it flat)          */
    uint64_t size;         /* plaintext bytes of the part                    */
    uint8_t md5[16];       /* the part ETag as raw bytes                     */
    uint32_t part_number;
    uint8_t encrypted;     /* frames under the upload key (SSE multipart)    */
} mxec_multipart_part;

/* complete_multipart_chunked (filesystem.rs:1147-1310): parts concatenated,
 * re-chunked, parity, manifest.json; etag_out receives "<hex md5 of the
 * parts' raw MD5s>-<n_parts>" (unquoted, :1240-1244).  The composite
 * x-amz-checksum is mxec_body_sums_batch over the parts' raw checksums. */
int mxec_complete_multipart_chunked(mxec_ctx* ctx, const char* ec_dir,
                                    uint64_t chunk_size, uint32_t parity_shards,
                                    const mxec_multipart_part* parts, uint32_t n_parts,
                                    char etag_out[48]);

/* complete_multipart_chunked_encrypted (filesystem.rs:1315-1560): encrypted
 * parts are decrypted with upload_key (AADs of "PART" 0 upload_id 0
 * part_number_le4 0, :147-163), the recombined plaintext re-encrypted under
 * the object key as in mxec_put_object_chunked_encrypted, chunked, parity,
 * manifest with plaintext_size; the same ETag. */
int mxec_complete_multipart_chunked_encrypted(mxec_ctx* ctx, const char* ec_dir,
                                              uint64_t chunk_size, uint32_t parity_shards,
                                              const mxec_multipart_part* parts, uint32_t n_parts,
                                              const uint8_t upload_key[32], const char* upload_id,
                                              const uint8_t key[32], const uint8_t nonce_prefix[4],
                                              const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                                              char etag_out[48]);

/* The two completions above as streams (the reference's loops hold one I/O
 * buffer, one frame and one chunk): no part and no body is buffered.  After
 * MXEC_OK ec_dir holds byte for byte the files and manifest.json the buffered
 * call writes for the same arguments, and etag_out the same string.
 * window_bytes is the writer's (mxec_writer_open below); 0 is the default.
 *
 * Every part file is opened and its size taken first (and closed again: the
 * feed holds open only the files one step draws from).  The body's length is
 * the sum of the plain parts' file sizes (part.size is ignored for a plain
 * part, as in the reference and the buffered call) and the encrypted parts'
 * `size`.  Decided before anything is created: a missing file (MXEC_E_IO); an
 * encrypted part without upload_key / upload_id, or given to the plain call
 * (MXEC_E_INVALID_ARG, the buffered texts); an encrypted part whose file is
 * shorter than mxec_frames_len(size, 65536) (MXEC_E_INTEGRITY "truncated
 * encrypted frame"; trailing bytes are ignored); the writer's own open errors
 * (chunk_size == 0, k + m > 255).  A part file that yields fewer bytes than
 * its size said is MXEC_E_IO.
 *
 * mxec_complete_multipart_streamed reads each part in pieces of at most 1 MiB
 * into mxec_writer_write.  The encrypted call opens mxec_writer_open_encrypted
 * over the body's length; a plain part goes through that writer's host path;
 * an encrypted part's frames go up, 16 at a time, into a ciphertext bounce in
 * HBM, and one launch of mxec_frames_decrypt_ring_device per 16 frames --
 * shared by consecutive encrypted parts, one job per part -- decrypts them
 * under the upload key straight into the writer's plaintext ring at the body
 * offset, where the writer's encrypt launches find them: the plaintext never
 * exists on the host and crosses no bus.  Mixed parts are allowed
 * (filesystem.rs:1375-1387).  The frame statuses come down behind each launch
 * and are all checked before any parity file or the manifest is written: a
 * bad frame is MXEC_E_INTEGRITY with mxec_frames_decrypt's texts.
 * On any failure after the writer opened no manifest.json exists; chunk files
 * written so far may remain, as after the reference's loop.
 * Memory: host, the writer's pieces, two page-locked ciphertext pieces of
 * 16 frames (1 049 024 bytes) each, one 1 MiB read buffer and the manifest's
 * entries; HBM, the writer's, plus the 2.1 MB ciphertext bounce and a second
 * 12.6 KiB key table.  None grows with the object. */
int mxec_complete_multipart_streamed(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                     uint32_t parity_shards, const mxec_multipart_part* parts,
                                     uint32_t n_parts, uint64_t window_bytes, char etag_out[48]);
int mxec_complete_multipart_streamed_encrypted(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                     uint32_t parity_shards, const mxec_multipart_part* parts,
                                     uint32_t n_parts, const uint8_t upload_key[32], const char* upload_id,
                                     const uint8_t key[32], const uint8_t nonce_prefix[4],
                                     const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                                     uint64_t window_bytes, char etag_out[48]);

/* put_object_chunked (filesystem.rs:686-773) as a push stream: the body is
 * written in pieces of any size and never buffered whole -- the write-side
 * counterpart of mxec_reader_*.  The handle is an opaque `mxec_writer`, passed
 * as void* (as mxec_scrub_object passes its report).
 *
 * mxec_writer_open (filesystem.rs:686-708): total_len is the body's length,
 * declared up front (Content-Length, x-amz-decoded-content-length, or the sum
 * of a multipart upload's parts): k = ceil(total_len / chunk_size), 1 for an
 * empty body, and the encoding matrix depends on k.  plaintext_size:
 * UINT64_MAX, or manifest.plaintext_size (a caller streaming an
 * encrypt-then-EC frame stream).  window_bytes: HBM for data chunks in
 * flight, 0 = default (4 chunks); at least 2 * chunk_size is used.  One device
 * of the context is chosen here, round robin, and kept.  chunk_size == 0 is
 * MXEC_E_INVALID_ARG; k + m > 255 with parity is MXEC_E_TOO_MANY_SHARDS_255
 * with put_object_chunked's text.  Unlike the reference, which writes every
 * data chunk before compute_and_write_parity hits that guard, both fail here
 * and nothing is created: k is known before the first byte.
 *
 * mxec_writer_write (filesystem.rs:709-737): any len, any split; returns once
 * buf is reusable.  Bytes go to the chunk's file ({index:06}) and to the
 * chunk's slot of the HBM window; a completed chunk's SHA-256 and its fold
 * into the running parity (mxec_encode_update_strided_device, count = 1) are
 * queued and the call returns.  It waits for the GPU only when the window is
 * full: the oldest chunk's hash or parity pass has not finished.
 *
 * mxec_writer_finish (filesystem.rs:738-773): takes exactly total_len bytes
 * written (else MXEC_E_INVALID_ARG "body ended at X of Y declared bytes"),
 * drains, writes the parity files, then manifest.json last.  ec_dir then
 * holds exactly the files and manifest bytes mxec_put_object_chunked writes
 * for the concatenated body, however it was split.
 *
 * mxec_writer_close: always; without a finish no manifest exists and the
 * chunk files written so far are left.
 *
 * Errors poison the writer: writing past total_len (MXEC_E_INVALID_ARG), an
 * I/O or device error, a short finish -- every later write or finish returns
 * that error and no manifest is ever written.
 * Memory: host, two page-locked staging pieces of at most 1 MiB each (body
 * bytes on their way up, parity rows on their way down to their files) and
 * the manifest's entries, one digest per chunk; HBM, the window plus
 * 2 * m * chunk_size.  No buffer of either grows with total_len or holds more
 * than a piece of a chunk on the host.
 * Threads: one writer is used by one thread at a time; any number of writers
 * run concurrently on a context, each on a stream of its own, sharing a slot
 * lock only within a call.
 *
 * mxec_writer_open_sums / mxec_writer_sums: the loop's Md5 and ChecksumHasher
 * (filesystem.rs:700-725) and PutResult.etag / checksum_value (:775-777)
 * inside the writer.  `which` (MXEC_SUM_*) names the body digests wanted;
 * 0 is mxec_writer_open.  They advance on a stream of their own in runs over
 * bytes already in the window (mxec_body_sums_update_device): a run ends at a
 * chunk's end or at each whole MiB of a chunk and is queued as soon as its
 * last byte's upload is, so however small the writes are there is one launch
 * per run, and a body that arrives slower than the chains run pays at most
 * one run's chain after its last byte.  A window slot is reused once its
 * chunk's last run has finished too; write() still waits for the GPU only
 * when the window is full.  finish() also brings the 76-byte record down (an
 * empty body is one run of length 0).  mxec_writer_sums after a successful
 * finish copies the requested fields into *out (the others are left
 * untouched): what mxec_put_object_chunked_sums returns for the concatenated
 * body.  Before a finish it is MXEC_E_INVALID_ARG ("sums before finish"); on
 * a poisoned writer, the poisoning error; with which == 0, MXEC_OK and
 * nothing written.
 * The digests are of the bytes written: a caller who pushes an
 * encrypt-then-EC frame stream (plaintext_size set) gets the frame stream's
 * digests, not the plaintext's as mxec_put_object_chunked_encrypted returns.
 * One lone fast body pays for them: its wall time becomes the slowest
 * requested chain's (MD5: about 13 ns per byte against 1.1 on a CPU core);
 * they pay with many bodies in flight.
 *
 * mxec_writer_open_encrypted (put_object_chunked_encrypted,
 * filesystem.rs:835-1060, as a push stream; FrameEncryptor, crypto.rs:94-117):
 * the caller writes plaintext, exactly plaintext_len bytes in pieces of any
 * size, and the writer encrypts.  The frame stream has
 * mxec_frames_len(plaintext_len, 65536) bytes: k, the chunk lengths and the
 * shard-count guards come from that length, decided here before anything is
 * created.  Frames are 65536 bytes with first index 0, frame i's AAD =
 * SHA-256(aad_prefix || i as u64 LE) (build_frame_aad, filesystem.rs:118-128).
 * After finish, ec_dir holds byte for byte what
 * mxec_put_object_chunked_encrypted writes for the concatenated body:
 * total_size = frame-stream bytes, plaintext_size = plaintext_len; an empty
 * body is one empty chunk, no parity, plaintext_size 0.  `which` /
 * mxec_writer_sums give the digests of the plaintext, as the buffered call
 * does.  mxec_writer_write, _finish, _sums and _close take the handle
 * unchanged; the error contract is the plain writer's, the over-run and
 * short-finish texts in plaintext bytes.  A null key or nonce_prefix, or
 * aad_prefix_len without aad_prefix, is MXEC_E_INVALID_ARG, as is a
 * plaintext_len whose frame stream does not fit in 64 bits.
 * Data path: plaintext goes through the staging pieces into a ring of four
 * 1 MiB stretches in HBM, not into the window, and the digest runs read it
 * there.  With a stretch's last byte (or the body's) one launch of the GCM
 * kernel's window form (mxec_frames_encrypt_window_device) encrypts its 16
 * frames straight into the chunk slots, behind the upload: one launch per MiB
 * however small the writes are.  Its AADs are hashed on the host and go up in
 * front of it; the key schedule and GHASH tables are prepared once at open and
 * stay in HBM until close, when the host copies of key and tables are zeroed.
 * The ciphertext comes down through two more page-locked pieces (at most
 * 1 MiB each) and goes to the chunk files a piece or two behind the encrypt;
 * finish() drains them.  A completed ciphertext chunk is hashed and folded as
 * in the plain writer.  A stretch is reused once its launch and digest run
 * have finished, a slot once its chunk's hash, fold and download have.
 * window_bytes: as above, but never fewer slots than one launch's
 * 1 049 024 stream bytes touch (ceil(1 049 024 / chunk_size) + 1, or all k).
 * Memory: host, four page-locked pieces and the manifest's entries; HBM, the
 * window, 2 * m * chunk_size of parity, the 4 MiB plaintext ring and 12.6 KiB
 * of key tables.  None grows with plaintext_len. */
typedef struct mxec_writer mxec_writer;
int mxec_writer_open(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                     uint32_t parity_shards, uint64_t total_len, uint64_t plaintext_size,
                     uint64_t window_bytes, void** out);
int mxec_writer_open_sums(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                          uint32_t parity_shards, uint64_t total_len, uint64_t plaintext_size,
                          uint64_t window_bytes, uint32_t which, void** out);
int mxec_writer_open_encrypted(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                               uint32_t parity_shards, uint64_t plaintext_len,
                               const uint8_t key[32], const uint8_t nonce_prefix[4],
                               const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                               uint64_t window_bytes, uint32_t which, void** out);
int mxec_writer_write(void* w, const uint8_t* buf, uint64_t len);
int mxec_writer_finish(void* w);
int mxec_writer_sums(void* w, mxec_body_sums* out);
void mxec_writer_close(void* w);

/* GET of a whole EC object (VerifiedChunkReader over manifest.json,
 * chunk_reader.rs:35-152): verified chunks, RS recovery of bad ones.
 * out must hold manifest total_size bytes; *out_len receives it.
 * offset/length select a range as with_range (:52-82); length UINT64_MAX = to
 * the end.  Chunks the range covers whole are read straight into out and
 * verified there, so out must not be touched by anyone else during the call;
 * on an error *out_len is the number of bytes served before the bad chunk
 * (the streaming reader's prefix) and the bytes of out past it are
 * unspecified. */
int mxec_get_object_chunked(mxec_ctx* ctx, const char* ec_dir, uint64_t offset,
                            uint64_t length, uint8_t* out, uint64_t out_cap,
                            uint64_t* out_len);

/* GET / ranged GET of an encrypt-then-EC object (filesystem.rs:1618-1630,
 * :1700-1725): the frames covering [offset, offset + length) of the
 * plaintext (FrameDecryptor::ciphertext_offset / for_range) are read through
 * the verified chunk reader, decrypted (AADs SHA-256(aad_prefix || i LE)) and
 * the range copied to out.  frame_size = the object's encryption chunk_size;
 * plaintext_size = ObjectMeta.size, or UINT64_MAX for the manifest's
 * plaintext_size; length UINT64_MAX = to the end. */
int mxec_get_object_chunked_encrypted(mxec_ctx* ctx, const char* ec_dir, const uint8_t key[32],
                                      const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                                      uint32_t frame_size, uint64_t plaintext_size,
                                      uint64_t offset, uint64_t length, uint8_t* out,
                                      uint64_t out_cap, uint64_t* out_len);

/* VerifiedChunkReader (chunk_reader.rs:12-276) as a pull stream.
 * mxec_reader_open = new (:35-49) when offset == 0 and length == UINT64_MAX,
 * with_range (:52-82) otherwise.  mxec_reader_read = poll_read (:228-276):
 * returns bytes copied (> 0), 0 at the end, or a negative error code; chunks
 * are verified against the manifest (size + SHA-256) in GPU batches of up to
 * `batch_bytes` (0 = 64 MiB), bad chunks of a batch are rebuilt in one decode
 * when the manifest has parity, and an unrecoverable chunk fails the read
 * that reaches it — after every byte before it was served, as the reference
 * aborts mid-stream. */
typedef struct mxec_reader mxec_reader;
int mxec_reader_open(mxec_ctx* ctx, const char* ec_dir, uint64_t offset,
                     uint64_t length, uint64_t batch_bytes, mxec_reader** out);
int64_t mxec_reader_read(mxec_reader* r, uint8_t* buf, uint64_t cap);
void mxec_reader_close(mxec_reader* r);

/* mxec_reader_open_encrypted (get_object / get_object_range of an
 * encrypt-then-EC object, filesystem.rs:1618-1630, :1700-1725, as a pull
 * stream: FrameDecryptor::for_range over VerifiedChunkReader,
 * crypto.rs:186-420): the read-side counterpart of mxec_writer_open_encrypted.
 * mxec_reader_read and mxec_reader_close take the handle unchanged.  offset
 * and length are plaintext coordinates (length UINT64_MAX = to the end);
 * plaintext_size = ObjectMeta.size, or UINT64_MAX for the manifest's
 * (MXEC_E_JSON when it has none); frame_size any positive multiple of 16 below
 * 2^31 - 256; batch_bytes as in mxec_reader_open.  The argument errors are
 * mxec_get_object_chunked_encrypted's.
 *
 * Concatenated, the bytes read() returns are exactly what
 * mxec_get_object_chunked_encrypted returns for the same arguments, for every
 * (offset, length), every read size and every batch_bytes.
 *
 * Failures stream.  A frame that fails (index, tag, truncation) or an
 * unrecoverable chunk under a frame fails the read that reaches it, after
 * every plaintext byte of the range in front of the failing frame was
 * returned.  Plaintext of a frame whose tag did not verify is never returned,
 * not even partially.  After an error every later read returns it again.
 * The chunk reader's errors are verbatim ("checksum mismatch on chunk ...",
 * "failed to read chunk ...", size mismatch, too few shards);
 * MXEC_E_INTEGRITY carries crypto.rs's three messages, "frame index mismatch:
 * expected E, got G" with the stored index, which the reader fetches from HBM.
 * Chunks with parity are repaired as the plain reader repairs them (its host
 * path; the rebuilt chunk goes up into its slot) and decrypted after that.
 *
 * Data path: at open the key schedule and GHASH tables are prepared once and
 * stay in HBM until close, when the host copies of key and tables are zeroed.
 * The frames of the range are [offset / frame_size, (end - 1) / frame_size],
 * whole, from FrameDecryptor::ciphertext_offset on.  A round takes the next
 * chunks of those stream bytes up to batch_bytes (at least one), reads them
 * from their files through two page-locked pieces (at most 1 MiB each) into
 * their slots of a ring in HBM (chunk j in slot j % slots), hashes them where
 * they lie and compares with the manifest.  One launch of the GCM kernel's
 * decrypt window form (mxec_frames_decrypt_window_device) then decrypts every
 * frame that is whole in verified chunks; its AADs are hashed on the host and
 * go up in front of it.  The statuses come down first, then only the
 * plaintext the range still wants (a ranged read skips the head of its first
 * frame and the tail of its last), through one more page-locked piece as
 * read() asks for it.  A frame cut by the round's end waits for the next
 * round, and its chunks' slots are not reused before it is decrypted: the ring
 * never has fewer slots than one frame can touch plus one, or all the range's
 * chunks.  Every ciphertext byte is uploaded once.
 * Memory: host, three page-locked pieces, the AADs and statuses of one launch;
 * HBM, the ring (one round plus one frame of ciphertext), one launch's
 * plaintext and 12.6 KiB of key tables.  None grows with the object.
 * Threads: one reader is used by one thread at a time; any number of readers
 * run concurrently on a context, each on a stream of its own. */
int mxec_reader_open_encrypted(mxec_ctx* ctx, const char* ec_dir, const uint8_t key[32],
                               const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                               uint32_t frame_size, uint64_t plaintext_size,
                               uint64_t offset, uint64_t length, uint64_t batch_bytes,
                               mxec_reader** out);

/* try_reconstruct_data_chunk (chunk_reader.rs:157-226) over ec_dir's files and
 * manifest.json: out receives chunks[target].size bytes. */
int mxec_try_reconstruct_data_chunk(mxec_ctx* ctx, const char* ec_dir,
                                    uint32_t target, uint8_t* out,
                                    uint64_t out_cap, uint64_t* out_len);

/* ---- scrub / heal of one EC object ---------------------------------------
 * The reference has no scrubber (no heal-on-read, no background repair): rot
 * in a shard nobody reads -- parity on every healthy GET -- stays until a
 * reconstruct needs it.  mxec_scrub_object checks one `{key}.ec` directory
 * (one stripe: k = chunk_count data shards of chunk_size bytes plus the
 * manifest's parity shards, as mxec_try_reconstruct_data_chunk treats it)
 * and can rewrite damaged shards.
 *   flags   MXEC_SCRUB_PARITY   if every shard file is present with the
 *                               manifest's size, mxec_verify over them: a
 *                               cheap first pass that cannot say which shard
 *                               is at fault; skipped (parity_consistent -1)
 *                               for an object without parity or with a
 *                               missing / wrong-sized file;
 *           MXEC_SCRUB_DIGESTS  SHA-256 of every present shard, parity
 *                               included, against the manifest (as the GET
 *                               compares: a recorded digest that is not 64
 *                               lower-case hex digits matches nothing);
 *           MXEC_SCRUB_HEAL     implies DIGESTS; 1 <= damaged <= m: every
 *                               damaged shard, data and parity, is rebuilt
 *                               from the verified ones, hashed, and -- only
 *                               if every rebuilt digest equals the
 *                               manifest's -- written to a temporary name in
 *                               ec_dir, fsynced and renamed over its final
 *                               name.  manifest.json is never rewritten.
 * Every mode sizes every shard file as the GET path does; a missing or
 * wrong-sized file is marked in shard_state in every mode.
 *   verdict MXEC_SCRUB_CLEAN, _DAMAGED (not healed: HEAL not asked), _HEALED,
 *           or _UNRECOVERABLE (HEAL asked, but more than m shards damaged or
 *           a rebuilt shard's digest disagrees with the manifest: no file is
 *           created, changed or removed).
 * Returns MXEC_OK whenever the scrub itself ran -- damage is reported in
 * *out, not as an error; manifest, I/O and RS-init errors as from
 * mxec_get_object_chunked.  Thread-safe: a scrubber may run several objects
 * from several threads.  `out` points at a mxec_scrub_report. */
#define MXEC_SCRUB_PARITY 1u
#define MXEC_SCRUB_DIGESTS 2u
#define MXEC_SCRUB_HEAL 4u
#define MXEC_SCRUB_CLEAN 0
#define MXEC_SCRUB_DAMAGED 1
#define MXEC_SCRUB_HEALED 2
#define MXEC_SCRUB_UNRECOVERABLE 3
#define MXEC_SHARD_OK 0
#define MXEC_SHARD_MISSING 1
#define MXEC_SHARD_BAD_SIZE 2
#define MXEC_SHARD_BAD_DIGEST 3
#define MXEC_SHARD_HEALED 0x80 /* or-ed into the state of a rewritten shard */
struct mxec_scrub_report {
    uint32_t k, m, verdict, n_damaged, n_healed;
    int32_t parity_consistent; /* 1 / 0, -1 = not checked */
    uint64_t parity_first_bad; /* lowest mismatching offset over all rows, or MXEC_VERIFY_OK */
    uint8_t shard_state[256];  /* first k+m entries */
};
typedef struct mxec_scrub_report mxec_scrub_report;
int mxec_scrub_object(mxec_ctx* ctx, const char* ec_dir, uint32_t flags, void* out);

/* ---- locate / fast heal of one EC object ----------------------------------
 * The scrub's cheap pass, naming the shard: reads the manifest and sizes
 * every shard file exactly as mxec_scrub_object does, then runs mxec_locate
 * over them -- no SHA-256 of any present shard.
 *   outcome MXEC_LOCATE_CLEAN, _ONE (`shard` is the damaged one), _MANY, or
 *           _SKIPPED: no parity location is possible (m < 2, m > 8, or a
 *           shard file missing / wrong-sized) -- run mxec_scrub_object.
 *   flags   MXEC_LOCATE_F_HEAL  on outcome ONE, that shard alone is rebuilt
 *           from the others, the rebuilt shard alone is hashed against the
 *           manifest's digest, and on equality written like a scrub's heal
 *           (temporary name, fsync, rename): healed = 1.  On disagreement,
 *           or a digest that is not 64 lower-case hex digits, nothing is created, changed or
 *           removed and healed = 0: fall back to the scrub's HEAL.
 * Returns MXEC_OK whenever the pass ran; manifest, I/O and RS-init errors as
 * from mxec_scrub_object; unknown flags MXEC_E_INVALID_ARG.  `out` points at
 * a mxec_locate_report. */
#define MXEC_LOCATE_SKIPPED 3
#define MXEC_LOCATE_F_HEAL 1u
struct mxec_locate_report {
    uint32_t k, m, outcome, shard; /* shard valid when outcome == MXEC_LOCATE_ONE */
    uint64_t first_bad, n_bad;
    uint32_t healed, reserved; /* healed: 1 iff the shard file was replaced */
};
typedef struct mxec_locate_report mxec_locate_report;
int mxec_locate_object(mxec_ctx* ctx, const char* ec_dir, uint32_t flags, void* out);

#ifdef __cplusplus
}
#endif
#endif /* MAXIO_EC_H */
