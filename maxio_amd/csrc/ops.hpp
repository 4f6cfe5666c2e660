// ops.hpp — device-pointer level operations shared by every C entry point.
#pragma once

#include <chrono>
#include <cstdint>
#include <exception>
#include <mutex>
#include <new>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "decode_tables.hpp"
#include "gf256.hpp"
#include "rs_plan.hpp"
#include "runtime.hpp"

namespace mxec {

// RsObject and RsMixedObject, what run_rs and run_rs_mixed take: rs_plan.hpp,
// with the host-only plan of their launches and descriptor tables.

// Applies each object's matrix; all objects share (k, r, shard_size).
// arena: take the descriptor tables from it instead of the slot's ring (many
// launches in flight, see pipeline.hpp).
// tune = false: the default grid, and the grid tuner neither picks nor
// records (the batch allocator's placement probes, placement.cpp).
int run_rs(Device& dev, Slot& slot, hipStream_t s, uint64_t shard_size, int k, int r,
           const std::vector<RsObject>& objs, DescArena* arena = nullptr, bool tune = true,
           uint32_t max_blocks = 0);

// Grid tuner of large uniform RS launches (runtime.hpp GridTuner):
// rs_grid_pick sets *bpc (0 = the default grid) and, while a shape is still
// being tuned, hands back a trial whose events the caller records around
// the launch and passes to rs_grid_record.  rs_grid_in_use: the workgroups
// per CU a shape runs at now (0 while undecided).  MXEC_RS_TUNE=0 disables,
// MXEC_RS_BPC fixes the grid.
int rs_grid_pick(Device& dev, int k, int r, uint64_t shard_size, double gb, uint32_t* bpc,
                 GridTuner::Trial* trial);
void rs_grid_record(Device& dev, int k, int r, uint64_t shard_size, const GridTuner::Trial& trial);
int rs_grid_in_use(Device& dev, int k, int r, uint64_t shard_size);
void rs_grid_release(Device& dev);

// Applies each object's matrix, objects grouped by r (map key).  Per r, the
// objects whose pointers are all 16-byte aligned (r <= 8) share one grouped
// launch (rs_apply_fast<GRP>), every grouped launch's tables in one upload;
// when two or more such groups all have r <= 4 they run as ONE multi-r
// launch instead (rs_apply_multi; MXEC_RS_MULTI=0 disables).  The others run
// one run_rs per (k, shard_size).  A lone uniform group runs the uniform
// kernel.
// max_blocks (here and in run_rs): a cap on each launch's workgroups, the
// grid tuner left alone (0: the default grid, or mxec_open_test's cap).
int run_rs_mixed(Device& dev, Slot& slot, hipStream_t s, const std::map<int, std::vector<RsMixedObject>>& groups,
                 DescArena* arena = nullptr, uint32_t max_blocks = 0);

// SHA-256 of n device buffers.  digests_dev / expected_dev / ok_dev may be
// null (see ShaArgs).
// tmo_dev: a caller that reads back a 4-byte device word after the launch
// (and fails the call if it is not 0) passes this; only then may a batch of
// more 64-message groups than SIMDs take the stream form (sha256_kernel.hip),
// whose word it is.  Set to null when another form ran.
int run_sha(Device& dev, Slot& slot, hipStream_t s, const std::vector<const uint8_t*>& ptrs,
            const std::vector<uint64_t>& lens, uint8_t* digests_dev, const uint8_t* expected_dev,
            uint8_t* ok_dev, const std::vector<uint64_t>* exp_idx = nullptr,
            DescArena* arena = nullptr, int form = 0, const uint32_t** tmo_dev = nullptr);
// One piece of every listed chain (ShaPiece, kernels.hpp), lag pair form:
// message i is the next lens[i] bytes of the chain in state slot slots[i]
// (state_dev: [slots][8] words, carried between launches on one stream);
// totals[i] = the message's length if this piece ends it (digest into
// digests_dev[slots[i]]; with expected_dev, ok_dev[slots[i]] = digest ==
// expected_dev[slots[i]]), kShaNotFinal otherwise (lens[i] a multiple of 64).
// At most kShaLagMsgs messages per CU.
int run_sha_pieces(Device& dev, Slot& slot, hipStream_t s, const std::vector<const uint8_t*>& ptrs,
                   const std::vector<uint64_t>& lens, const std::vector<uint32_t>& slots,
                   const std::vector<uint64_t>& totals, uint32_t* state_dev, bool resume, uint8_t* digests_dev,
                   DescArena* arena, const uint8_t* expected_dev = nullptr, uint8_t* ok_dev = nullptr);

// SHA-256 digests (host out, n * 32 bytes) of n device-resident messages on
// `dev`, blocking; the caller's work on `s` must have produced them (the
// caller synchronises `s` first).  Concurrent small requests on one device
// share one launch on the combiner's stream (combiner.cpp); large ones run on
// the caller's slot and stream.
// The stream form pays once a batch has more 64-message groups than 3/4 of
// the SIMDs (sha256_kernel.hip kSplitMaxMessages).
inline bool sha_stream_size(uint64_t groups, uint64_t simds) { return groups * 4 > simds * 3; }

// `ready` (optional): an event the caller recorded on `s` when its messages
// were complete; without one the call records it now.  `after_launch`
// (optional) runs once the hash launch is queued, before the wait for its
// digests -- work to queue on `s` beside the hash; its status is the call's
// if the hash itself succeeded.
int sha256_combined(Device& dev, Slot& slot, hipStream_t s, const std::vector<const uint8_t*>& ptrs,
                    const std::vector<uint64_t>& lens, uint8_t* out, hipEvent_t ready = nullptr,
                    const std::function<int()>* after_launch = nullptr);
void combiner_stats(Device& dev, uint64_t* batches, uint64_t* messages);
// Whether a request of n messages goes through the combiner.
bool sha_combines(const Device& d, size_t n);

// Coefficient table of the (k, m) encoding matrix's parity rows.
int encode_coef(Device& dev, int k, int m, uint32_t* off);
// Coefficient table of a decode plan.
int decode_coef(Device& dev, const DecodePlan& plan, bool data_only, uint32_t* off);

// Decode plan + table offset for one erasure pattern (present: k+m flags),
// memoised per device so a batch that repeats patterns pays one hash lookup
// per object.  *plan is null when fewer than k shards are present.
int decode_plan(Device& dev, int k, int m, const uint8_t* present, bool data_only,
                std::shared_ptr<const DecodePlan>* plan, uint32_t* off);

// The decode launch of every reconstruct: bytes [off, off + pw) of each
// item's missing shards from its decode plan (looked up from its present
// flags as they stand; none for an item short of k shards or with S <= off),
// in one grouped launch on s (decode_tables.hpp, run_rs_mixed with `arena`
// and `max_blocks`), under with_stable_coef.  plans[t] is item t's plan.
int decode_step(Device& dev, Slot& slot, hipStream_t s, std::vector<DecodeItem> items, bool data_only,
                std::vector<std::shared_ptr<const DecodePlan>>& plans, uint64_t off = 0,
                uint64_t pw = ~uint64_t(0), DescArena* arena = nullptr, uint32_t max_blocks = 0);

// Host-API staging: shard slots are this many bytes apart on the device.
constexpr uint64_t kSlotAlign = 256;
inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// Runs an entry point body; no C++ exception crosses the C ABI.  Returns
// what the body returns (int, or int64_t for a byte count or an error).
template <class F>
auto guarded(F&& f) -> decltype(f()) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return set_error(MXEC_E_OOM, "host allocation failed");
    } catch (const std::exception& e) {
        return set_error(MXEC_E_INVALID_ARG, e.what());
    } catch (...) {
        return set_error(MXEC_E_INVALID_ARG, "unknown exception");
    }
}

// A device of the context (dev_index < 0: round robin) with one of its slots
// locked for the duration of a call.
// On the way out (any path, the lock still held) it waits for DMAs still
// reading the caller's page-locked buffers (Slot::borrowed).
struct DevScope {
    Device* d = nullptr;
    std::unique_lock<std::mutex> lk;
    Slot* slot = nullptr;
    DevScope() = default;
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;
    ~DevScope() {
        if (slot && slot->borrowed) {
            const std::string keep = last_error();  // an early return's message stays
            (void)slot_wait(*slot, slot->borrowed);
            if (slot->borrowed) {  // the wait itself failed: drain the device
                (void)hipStreamSynchronize(slot->borrowed);
                slot->borrowed = nullptr;
            }
            set_error(0, keep);
        }
    }
    int open(mxec_ctx* ctx, int dev_index) {
        if (!ctx) return set_error(MXEC_E_INVALID_ARG, "null context");
        d = pick_device(&ctx->c, dev_index);
        if (!d) return set_error(MXEC_E_INVALID_ARG, "no such device in context");
        MXEC_HIP(hipSetDevice(d->id));
        slot = &lock_slot(*d, lk);
        return MXEC_OK;
    }
};


// MXEC_PIPE_COPY (knobs.hpp): whether a host-pointer call's copies of
// mxec_host_alloc memory may go by CU-wave copy kernels -- the reconstruct /
// hash (GET) paths under auto and waves, the encode (PUT) path under waves
// only (copy_watch.hpp has the measurements behind the split).
inline bool copy_waves_get(const Device& d) {
    if (!d.kn) return false;
    if (d.kn->pipe_copy == 1) return true;
    if (d.kn->pipe_copy != 2) return false;
    const int64_t now = std::chrono::duration_cast<std::chrono::nanoseconds>(
                            std::chrono::steady_clock::now().time_since_epoch()).count();
    return now < d.waves_up_until_ns.load() || now < d.waves_down_until_ns.load();
}
inline bool copy_waves_put(const Device& d) { return d.kn && d.kn->pipe_copy == 1; }

// PUT body digests of device-resident bodies into mxec_body_sums records
// (sums.cpp); enqueued on s.
// upd: the update form (mxec_body_sums_update_device) -- ptrs / lens are the
// next piece of every body, whose state is the record at state_dev +
// i * MXEC_SUMS_STATE_BYTES; out_dev is written with MXEC_SUMS_F_FINAL only.
// arena: the tables from it instead of the slot's ring, whose entries a
// caller with many runs queued behind a slow chain would wait for.
struct SumsUpdate {
    uint8_t* state_dev;
    uint32_t flags;  // MXEC_SUMS_F_*
};
int run_body_sums(Device& d, Slot& slot, hipStream_t s, const std::vector<const uint8_t*>& ptrs,
                  const std::vector<uint64_t>& lens, uint32_t which, uint8_t* out_dev, uint64_t stride,
                  const SumsUpdate* upd = nullptr, DescArena* arena = nullptr);

// AES-256-GCM frames (gcm.cpp).  gcm_prepare_key fills a data key's tables
// (kernels.hpp GcmKey: key schedule, H^1..H^256, the position table of H^256;
// ~30 us of host work): the frame entry points do it per call, a caller with
// many launches under one key does it once and keeps the record in HBM.
// gcm_encrypt_window: the launch of mxec_frames_encrypt_window_device over
// arguments gcm_window_check has passed, enqueue-only; key_dev = that
// resident record (q.key is then not read), or null to prepare q.key here;
// arena = where the launch's tables go instead of the slot's ring.
// gcm_decrypt_window: the same for mxec_frames_decrypt_window_device (checked
// with decrypt = true: out_dev is then the contiguous side, in_dev ignored);
// status_dev takes a status per frame, written on s like the plaintext.
// gcm_ring_check / gcm_decrypt_ring: the checks and the launch of
// mxec_frames_decrypt_ring_device, enqueue-only; key_dev = one resident
// record that every job runs under (the jobs' keys are then not read).
// gcm_frame_fail: MXEC_E_INTEGRITY with crypto.rs's text for a frame status
// (2: index mismatch with both indices, else the authentication error).
struct GcmKey;
int gcm_frame_fail(int32_t status, uint64_t expected, uint64_t got);
void gcm_prepare_key(const uint8_t key[32], GcmKey& out);
int gcm_window_check(const mxec_frames_job& q, const mxec_frames_window& w, bool need_key, bool decrypt = false);
int gcm_encrypt_window(Device& d, Slot& slot, hipStream_t s, const GcmKey* key_dev, const mxec_frames_job& q,
                       uint64_t stream_off, const mxec_frames_window& w, DescArena* arena = nullptr);
int gcm_decrypt_window(Device& d, Slot& slot, hipStream_t s, const GcmKey* key_dev, const mxec_frames_job& q,
                       uint64_t stream_off, const mxec_frames_window& w, int32_t* status_dev,
                       DescArena* arena = nullptr);
int gcm_ring_check(const mxec_frames_job* jobs, uint64_t n_jobs, const uint64_t* ring_off, const mxec_frames_ring* ring,
                   const int32_t* status_dev, bool need_key);
int gcm_decrypt_ring(Device& d, Slot& slot, hipStream_t s, const GcmKey* key_dev, const mxec_frames_job* jobs,
                     uint64_t n_jobs, const uint64_t* ring_off, const mxec_frames_ring& ring, int32_t* status_dev,
                     DescArena* arena = nullptr);

// The device-side feed of an encrypted writer (storage_writer.cpp; not part of
// the ABI): the frames of encrypted multipart parts, decrypted under the
// upload key straight into the writer's plaintext ring.  writer_feed_key, once
// after mxec_writer_open_encrypted: the upload key's tables, resident until
// close.  writer_feed_frames: one launch step of part_plan.hpp's feed (planned
// over writer_ring_bytes of the body), src[j] the file of step.jobs[j]'s part;
// it takes the place of the mxec_writer_write of those plaintext bytes, may be
// mixed with such writes in body order, and poisons the writer like them.  A
// part frame that fails its check is MXEC_E_INTEGRITY with
// mxec_frames_decrypt's texts, from a later feed call or from finish().
struct FeedStep;
struct WriterFeedSrc {
    int fd;
    const char* path;  // for messages
    uint32_t part_number;
};
uint64_t writer_ring_bytes(uint64_t plain_len);
int writer_feed_key(void* writer, const uint8_t* upload_key, const char* upload_id);
int writer_feed_frames(void* writer, const FeedStep& step, const WriterFeedSrc* src);

// The multipart ETag (filesystem.rs:1240-1244): MD5 over the parts' raw MD5s,
// "-N" (storage_multipart.cpp).
int multipart_etag(mxec_ctx* ctx, const mxec_multipart_part* parts, uint32_t n_parts, char* etag_out);

// Creates the device's host-pipeline hub and its streams (pipe_hub.cpp),
// called by mxec_open for every device.
int pipe_open(Device& dev);

// filesystem.rs:1095 guard, then the crate's ReedSolomon::new checks.
int check_km(int k, int m);
// The guard's error (MXEC_E_TOO_MANY_SHARDS_255) with the reference's text.
int too_many_shards(uint64_t k, uint64_t m);

// chunk_reader.rs:203-206's error text for an object short of k shards.
inline std::string too_few_msg(int present, int k, int total) {
    return "too many missing/corrupt shards: only " + std::to_string(present) + " of " +
           std::to_string(k) + " required shards available (" + std::to_string(total - present) +
           " missing)";
}

// The shape check of every reconstruct: the crate's ReedSolomon::new checks,
// then its empty-shard error.
int reconstruct_shape(int k, int m, uint64_t shard_size);

// The end of a batch reconstruct: every object's status out, and the first
// failing object's as the call's own, with chunk_reader.rs's message.
// objs[o].k / .m: the objects' shapes; present: their flags, one object after
// another.
template <class Obj>
int reconstruct_status(const Obj* objs, uint64_t n_obj, const uint8_t* present, const std::vector<int32_t>& st,
                       int32_t* status_out) {
    int first_err = MXEC_OK;
    for (uint64_t o = 0; o < n_obj; ++o) {
        const int total = objs[o].k + objs[o].m;
        if (status_out) status_out[o] = st[o];
        if (st[o] != MXEC_OK && first_err == MXEC_OK) {
            int np = 0;
            for (int i = 0; i < total; ++i) np += present[i] != 0;
            first_err = st[o];
            set_error(first_err, too_few_msg(np, objs[o].k, total));
        }
        present += total;
    }
    return first_err;
}

// Coefficient-table offsets are valid while their generation's half of the
// device's table arena is not reused (runtime.hpp Device::coef_*): `collect`
// takes a batch's offsets (noting each table's generation and upload),
// `s` waits on the GPU for any of those tables still being uploaded,
// `launch` enqueues the kernels that read them on `s`; then, under the arena's lock,
// either every generation used is still live and an event on `s` fences the
// batch (a later recycle of those halves waits for it), or one was recycled
// between `collect` and here, and the pair runs again.  A launch queued with
// a recycled half's offsets may have read foreign tables; its re-run is
// queued behind it on the same stream over the same outputs (the RS kernels
// read only inputs and write only outputs), so the last pass wins and the
// result is exact.
template <class C, class L>
int with_stable_coef(Device& d, hipStream_t s, C&& collect, L&& launch) {
    for (int attempt = 0; attempt < 8; ++attempt) {
        CoefUse use;
        CoefUse* outer = coef_use_swap(&use);
        int rc = collect();
        if (rc == MXEC_OK) rc = coef_wait_uploads(d, use, s);  // tables still on their way up
        if (rc == MXEC_OK) rc = launch();
        coef_use_swap(outer);
        MXEC_TRY(rc);
        bool live = true;
        MXEC_TRY(coef_fence(d, use, s, &live));
        if (live) return MXEC_OK;
    }
    return set_error(MXEC_E_INVALID_ARG,
                     "the coefficient tables of one batch exceed the device's table arena (recycled under it 8 times)");
}

}  // namespace mxec
